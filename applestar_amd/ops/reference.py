"""Plain-PyTorch definitions of every fused op.

These are (a) the implementation used for CPU tensors (``play.py --cpu``, CPU tests) and (b) the
fp32 golden oracle the HIP kernels are tested against.  Each function documents the reference
op sequence it reproduces.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

_ACTS = {
    None: lambda x: x,
    'relu': F.relu,
    'sigmoid': torch.sigmoid,
    'tanh': torch.tanh,
}


def act_fn(x, act):
    return _ACTS[act](x)


def linear(x, w, b=None, act=None):
    return act_fn(F.linear(x, w, b), act)


def layer_norm(x, w, b, residual=None, act=None, eps: float = 1e-5):
    if residual is not None:
        x = x + residual
    return act_fn(F.layer_norm(x, (x.shape[-1],), w, b, eps), act)


def conv2d(x, w, b, stride=1, padding=0, act=None, residual=None):
    y = F.conv2d(x, w, b, stride, padding)
    if residual is not None:
        y = y + residual
    return act_fn(y, act)


def gated_residual(y, g, sp, x):
    """GatedResBlock tail (module_utils.py:224-231): relu(tanh(y*sigmoid(g))*sp + x)."""
    return F.relu(torch.tanh(y * torch.sigmoid(g)) * sp + x)


def lnlstm_cell(x_proj_ln, h, c, w_hh, lnh_w, lnh_b, lnc_w, lnc_b):
    """One LayerNorm-LSTM step given the already-normalised input projection
    (lstm.py:138-153): gates = LN_i(x W_ih^T) + LN_h(h W_hh^T); (i,f,g,o); c' = LN_c(f c + i g);
    h' = o tanh(c').  The *normalised* c' is carried as state, as in the reference."""
    H = h.shape[-1]
    hg = F.layer_norm(h @ w_hh.t(), (4 * H,), lnh_w, lnh_b)
    gates = x_proj_ln + hg
    i, f, g, o = gates.chunk(4, dim=-1)
    c_new = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    c_new = F.layer_norm(c_new, (H,), lnc_w, lnc_b)
    h_new = torch.sigmoid(o) * torch.tanh(c_new)
    return h_new, c_new


def lnlstm_layer(x, h0, c0, w_ih, w_hh, lni_w, lni_b, lnh_w, lnh_b, lnc_w, lnc_b):
    """Whole-sequence LN-LSTM layer: x [T,B,I] -> out [T,B,H], (h_T, c_T).

    The input projection and its LayerNorm depend only on x, so they are hoisted out of the time
    loop into one [T*B, I] x [I, 4H] GEMM (the reference runs T small GEMMs).
    """
    T, B, _ = x.shape
    H = h0.shape[-1]
    xp = F.layer_norm(F.linear(x.reshape(T * B, -1), w_ih), (4 * H,), lni_w, lni_b).view(T, B, 4 * H)
    h, c = h0, c0
    outs = []
    for t in range(T):
        h, c = lnlstm_cell(xp[t], h, c, w_hh, lnh_w, lnh_b, lnc_w, lnc_b)
        outs.append(h)
    return torch.stack(outs, 0), h, c


def masked_attention(q, k, v, key_mask: Optional[torch.Tensor]):
    """Dense masked softmax attention (module_utils.py:88-111).
    q,k,v [B,H,N,D]; key_mask [B,N] bool (True = valid key). Scores of masked keys are -1e9."""
    d = q.shape[-1]
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(d)
    if key_mask is not None:
        s = s.masked_fill(~key_mask[:, None, None, :], -1e9)
    p = torch.softmax(s.float(), dim=-1).to(v.dtype)
    return torch.matmul(p, v)


def varlen_attention(qkv, cu_seqlens, max_len: int, num_heads: int, head_dim: int):
    """Packed varlen self-attention.  qkv [T, 3*H*D] laid out [q | k | v], each [H, D];
    cu_seqlens [S+1] int.  Returns [T, H*D].  Equivalent to ``masked_attention`` on the padded
    batch for every valid query row."""
    T = qkv.shape[0]
    HD = num_heads * head_dim
    seqlens = (cu_seqlens[1:] - cu_seqlens[:-1]).long()
    S = seqlens.numel()
    idx, valid = _pack_index(seqlens, max_len)
    pad = torch.zeros(S * max_len, 3 * HD, dtype=qkv.dtype, device=qkv.device)
    pad[valid] = qkv
    pad = pad.view(S, max_len, 3, num_heads, head_dim).permute(2, 0, 3, 1, 4)
    out = masked_attention(pad[0], pad[1], pad[2], valid.view(S, max_len))
    out = out.permute(0, 2, 1, 3).reshape(S * max_len, HD)
    return out[valid]


def qkv_attention(x, w, b, cu_seqlens, max_len: int, num_heads: int, head_dim: int):
    """Packed self-attention on the projection qkv = x W^T + b of the packed tokens x [T, K]."""
    return varlen_attention(F.linear(x, w, b), cu_seqlens, max_len, num_heads, head_dim)


def _pack_index(seqlens, max_len):
    ar = torch.arange(max_len, device=seqlens.device)
    valid = (ar[None, :] < seqlens[:, None]).reshape(-1)
    return None, valid


def sequence_mask(lengths: torch.Tensor, max_len: Optional[int] = None) -> torch.Tensor:
    if max_len is None:
        max_len = int(lengths.max())
    return torch.arange(max_len, device=lengths.device)[None, :] < lengths.reshape(-1, 1)


def scatter_connection(proj: torch.Tensor, x: torch.Tensor, y: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Scatter-add per-entity features into a map (module_utils.py:11-34, 'add' mode).
    proj [B,N,C] (already masked), x,y [B,N] integer coords -> [B,C,H,W]."""
    B, N, C = proj.shape
    xi = x.long().clamp(0, W - 1)
    yi = y.long().clamp(0, H - 1)
    flat = (yi * W + xi) + (torch.arange(B, device=proj.device) * (H * W))[:, None]
    out = torch.zeros(B * H * W, C, dtype=proj.dtype, device=proj.device)
    out.index_add_(0, flat.reshape(-1), proj.reshape(-1, C))
    return out.view(B, H, W, C).permute(0, 3, 1, 2)


def scatter_connection_ordered(proj: torch.Tensor, x: torch.Tensor, y: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """:func:`scatter_connection` with the summation order of the deterministic mode spelled out: each output element
    is the fp32 sum of its units' rows in ascending unit index, starting from the first contribution; pixels with no
    unit are +0.  A plain loop over the units (the observations and channels are independent); the bit-exact
    oracle of the native ordered kernel."""
    B, N, C = proj.shape
    pix = y.long().clamp(0, H - 1) * W + x.long().clamp(0, W - 1)
    rows = proj.float()
    out = torch.zeros(B, H * W, C, dtype=torch.float32, device=proj.device)
    seen = torch.zeros(B, H * W, dtype=torch.bool, device=proj.device)
    ar = torch.arange(B, device=proj.device)
    for u in range(N):
        p = pix[:, u]
        out[ar, p] = torch.where(seen[ar, p].unsqueeze(-1), out[ar, p] + rows[:, u], rows[:, u])
        seen[ar, p] = True
    return out.to(proj.dtype).view(B, H, W, C).permute(0, 3, 1, 2)


def gather_steps_grad_ordered(dout: torch.Tensor, labels: torch.Tensor, N1: int) -> torch.Tensor:
    """Gradient of ``key[b, labels[b, s], :]`` w.r.t. key [B, N1, C] in the deterministic mode's order: row n of
    observation b is the fp32 sum of dout[b, s, :] over the steps with labels[b, s] == n in ascending s (zero for a
    row no label names).  A plain loop over the steps; the bit-exact oracle of the native backward."""
    B, S, C = dout.shape
    lab = labels.long().clamp(0, N1 - 1)
    dkey = torch.zeros(B, N1, C, dtype=torch.float32, device=dout.device)
    ar = torch.arange(B, device=dout.device)
    for s in range(S):
        dkey[ar, lab[:, s]] = dkey[ar, lab[:, s]] + dout[:, s].float()
    return dkey.to(dout.dtype)


# ----------------------------------------------------------------------------- losses / RL math

def categorical_stats(logits: torch.Tensor, actions: torch.Tensor):
    """log-softmax, logp(action), probs — the quantities every RL loss head needs."""
    logp = torch.log_softmax(logits.float(), dim=-1)
    a_logp = logp.gather(-1, actions.long().unsqueeze(-1)).squeeze(-1)
    return logp, a_logp


def head_stats(logits: torch.Tensor, teacher: Optional[torch.Tensor], actions: torch.Tensor,
               successive: Optional[torch.Tensor] = None):
    """Per row of ``logits [..., C]``: (logp(action), entropy, KL(softmax(teacher) || softmax(logits))),
    fp32, shaped like ``actions`` (rl_loss.py:63-90, as_rl_utils.py:52-127).  KL is 0 without a teacher.
    With ``successive [..., C]`` a fourth result: KL(softmax(successive) || softmax(logits)) (DAPO)."""
    lp = torch.log_softmax(logits.float(), dim=-1)
    a = actions.long().clamp(0, logits.shape[-1] - 1)
    logp_a = lp.gather(-1, a.unsqueeze(-1)).squeeze(-1)
    ent = -(lp.exp() * lp).sum(-1)
    if teacher is None:
        kl = torch.zeros_like(ent)
    else:
        tlp = torch.log_softmax(teacher.float(), dim=-1)
        kl = (tlp.exp() * (tlp - lp)).sum(-1)
    if successive is None:
        return logp_a, ent, kl
    ulp = torch.log_softmax(successive.float(), dim=-1)
    return logp_a, ent, kl, (ulp.exp() * (ulp - lp)).sum(-1)


SL_INFO_KEYS = ('action_type_loss', 'delay_loss', 'queued_loss', 'selected_units_loss', 'target_unit_loss',
                'target_location_loss', 'selected_units_loss_norm', 'selected_units_end_flag_loss', 'action_type_acc',
                'delay_distance_L1', 'queued_acc', 'selected_units_iou', 'target_unit_acc',
                'target_location_distance_L2', 'total_loss')
SL_FLAT_HEADS = ('action_type', 'delay', 'queued', 'target_unit', 'target_location')


def sl_head_ce(logits: torch.Tensor, labels: torch.Tensor, eps: float = 0.0, row_on: Optional[torch.Tensor] = None,
               su=None, su_mask: bool = False):
    """Per row of ``logits [..., C]``: (cross entropy with label smoothing ``eps``, argmax = lowest index of the
    maximum), shaped like ``labels``; fp32 (float64 logits stay float64).  Labels are clamped to [0, C).
    Rows where ``row_on`` is 0 are switched off: their logits are not used (loss 0, argmax -1, zero gradient).
    Selected-units form, ``su = (su_len [b], su_on [b])`` with logits [b, S, C] and labels [b, S]: row (bi, si) is
    off when si >= su_len[bi] or su_on[bi] == 0; with ``su_mask`` every other labelled unit of the observation
    (labels[bi, j], j < su_len[bi] - 1, except the row's own label) reads as -1e9 (sl/loss.py _selected_units)."""
    C = logits.shape[-1]
    x = logits if logits.dtype == torch.float64 else logits.float()
    lab = labels.long()
    on = None
    if su is not None:
        su_len, su_on = su
        b, S = lab.shape
        su_len = su_len.long()
        on = sequence_mask(su_len, S) & (su_on != 0).unsqueeze(1)
        if su_mask:
            no_end = sequence_mask((su_len - 1).clamp(min=0), S) & (lab >= 0) & (lab < C)
            other = torch.where(no_end, lab, torch.full_like(lab, C))
            inset = torch.zeros(b, C + 1, dtype=torch.bool, device=x.device).scatter_(1, other, True)
            forbid = inset.unsqueeze(1).expand(b, S, C + 1).clone()
            forbid.scatter_(2, other.unsqueeze(2), False)
            x = x.masked_fill(forbid[:, :, :C], -1e9)
    elif row_on is not None:
        on = row_on != 0
    if on is not None:
        x = torch.where(on.unsqueeze(-1), x, torch.zeros_like(x))
    lp = torch.log_softmax(x, dim=-1)
    loss = -lp.gather(-1, lab.clamp(0, C - 1).unsqueeze(-1)).squeeze(-1)
    if eps > 0:
        loss = (1 - eps) * loss + eps * (-lp.mean(-1))
    amax = x.argmax(-1)
    if on is not None:
        loss = torch.where(on, loss, torch.zeros_like(loss))
        amax = torch.where(on, amax, torch.full_like(amax, -1))
    return loss, amax


def sl_loss_tail(losses, argmaxes, labels, masks, su_loss, su_labels, su_len, su_on, preds, ent_num, w, cr_scale,
                 n: int):
    """Everything of the supervised loss after the per-row cross entropies (sl/loss.py): (total, info [15] in
    ``SL_INFO_KEYS`` order).  ``losses / argmaxes / labels / masks``: the five flat heads (``SL_FLAT_HEADS``), [b] each;
    ``su_loss / su_labels`` [b, S], ``su_len / su_on`` [b]; ``preds`` [b, S] with ``ent_num`` [b] or both None (IoU 0);
    ``w`` [6] loss weights in HEADS order; ``cr_scale`` [1]: 0 = masked means, else world / total batch (every head's
    loss is then sum(loss * mask) * cr_scale); ``n``: unit ids 0 .. n-1 enter the IoU."""
    dt = su_loss.dtype
    dev = su_loss.device
    b, S = su_loss.shape
    cr = torch.as_tensor(cr_scale, device=dev).reshape(-1)[0].to(dt)
    cross = cr > 0
    w = torch.as_tensor(w, device=dev).to(dt)
    info = [None] * 15
    loss_slot, metric_slot = (0, 1, 2, 4, 5), (8, 9, 10, 12, 13)
    total = torch.zeros((), dtype=dt, device=dev)
    for f in range(5):
        m = (masks[f] != 0).to(dt)
        sm = m.sum()
        scale = torch.where(cross, cr, 1.0 / sm.clamp(min=1.0))
        lh = (torch.where(m > 0, losses[f].to(dt), torch.zeros_like(m))).sum() * scale
        p, a = argmaxes[f].long(), labels[f].long()
        if f == 0:
            met = (p == a).to(dt).mean()
        elif f == 3:
            met = ((p == a).to(dt) * m).sum() / (sm + 1e-6)
        elif f == 4:
            d = torch.stack([p % 160 - a % 160, p // 160 - a // 160], -1).to(dt)
            met = (d.pow(2).sum(-1).sqrt() * m).sum() / (sm + 1e-6)
        else:
            met = ((p - a).abs().to(dt) * m).sum() / (sm + 1e-6)
        info[loss_slot[f]], info[metric_slot[f]] = lh, met.detach()
        total = total + w[loss_slot[f]] * lh
    su_len = su_len.long()
    on = sequence_mask(su_len, S) & (su_on != 0).unsqueeze(1)
    sl = torch.where(on, su_loss, torch.zeros_like(su_loss))
    lsu = sl.sum() * torch.where(cross, cr, torch.ones((), dtype=dt, device=dev) / b)
    info[3] = lsu
    info[6] = (sl.sum() / (su_len.sum().to(dt) + 1e-6)).detach()
    info[7] = sl[torch.arange(b, device=dev), (su_len - 1).clamp(0, S - 1)].mean().detach()
    total = total + w[3] * lsu
    if preds is not None:
        pr = preds.long()
        is_end = pr == ent_num.long().unsqueeze(1)
        first_end = torch.where(is_end.any(1), is_end.to(dt).argmax(1) + 1, torch.full_like(su_len, S))
        pm = sequence_mask(first_end, S)
        P = torch.zeros(b, n + 1, dtype=torch.bool, device=dev)
        L = torch.zeros_like(P)
        P.scatter_(1, ((pr + 1) * pm).clamp(0, n), True)
        L.scatter_(1, ((su_labels.long() + 1) * sequence_mask(su_len, S)).clamp(0, n), True)
        inter = (P & L)[:, 1:].sum(1).to(dt)
        union = (P | L)[:, 1:].sum(1).to(dt)
        mo = (su_on != 0).to(dt)
        info[11] = (inter / (union + 1e-6) * mo).sum() / (mo.sum() + 1e-6)
    else:
        info[11] = torch.zeros((), dtype=dt, device=dev)
    info[14] = total
    return total, torch.stack([v.detach() for v in info])


def vtrace_advantages(clipped_rhos, clipped_cs, rewards, values, gamma: float = 1.0, lambda_: float = 1.0):
    """as_rl_utils.py:284-312. rhos/cs/rewards [T,B], values [T+1,B] -> advantages [T,B]."""
    T = rewards.shape[0]
    deltas = clipped_rhos * (rewards + gamma * values[1:] - values[:-1])
    vs = torch.empty_like(values)
    vs[-1] = values[-1]
    for t in range(T - 1, -1, -1):
        vs[t] = values[t] + deltas[t] + gamma * lambda_ * clipped_cs[t] * (vs[t + 1] - values[t + 1])
    return clipped_rhos * (rewards + gamma * vs[1:] - values[:-1])


def lambda_returns(rewards, values, gamma: float, lambdas):
    """generalized_lambda_returns / multistep_forward_view (as_rl_utils.py:157-218).
    rewards [T,B], values [T+1,B], lambdas scalar or [T,B] (last row ignored)."""
    T = rewards.shape[0]
    if not torch.is_tensor(lambdas):
        lambdas = torch.full_like(rewards, float(lambdas))
    boot = values[1:]
    out = torch.empty_like(rewards)
    out[-1] = rewards[-1] + gamma * boot[-1]
    disc = gamma * lambdas
    for t in range(T - 2, -1, -1):
        out[t] = rewards[t] + disc[t] * out[t + 1] + (gamma - disc[t]) * boot[t]
    return out


def upgo_returns(rewards, values):
    """as_rl_utils.py:265-281."""
    lam = (rewards + values[1:]) >= values[:-1]
    lam = torch.cat([lam[1:], torch.ones_like(lam[-1:])], 0).to(rewards.dtype)
    return lambda_returns(rewards, values, 1.0, lam)


def td_lambda_returns(rewards, values, gamma: float = 1.0, lambda_: float = 0.8):
    return lambda_returns(rewards, values, gamma, lambda_)
