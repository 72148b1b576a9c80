"""A float64 reference of the learner loss, the case generator of tests/test_loss_gpu.py, and the tests that
guard both (CPU only).

``reference_loss(outputs, batch, args)`` restates compute_loss after the network forward (train.py:220-258) and
compose_losses (train.py:188-215) from their formulas, in plain torch with autograd, in whatever dtype its
inputs have (the tests give it float64).  It takes what ``handyrl_amd.train.loss_terms`` takes:

* any number of players P, the policy with one row per step (Pp = 1) or one per player (Pp = P);
* an optional value head and an optional return head;
* the two-player zero-sum symmetrisation of the value (turn_based_training and P = 2);
* MC, TD, UPGO and VTRACE for the value targets and for the policy advantages, the recurrences as Python
  loops over T.

Besides the losses it returns, per loss, the sum of the magnitudes of the terms that were added up: the scale
against which the error of a float32 sum is judged.

It is pinned from two sides: by the reference project's recorded losses and gradients (tests/golden/loss.*) and
by the float32 CPU oracle (oracle.learner.loss_from_outputs, itself pinned by the same recordings) on generated
cases that the recordings do not hold: P in {1, 2, 3, 8}, both Pp, every head combination, every algorithm.
"""

import numpy as np
import pytest
import torch

from oracle import learner as ol

from tests.test_oracle_learner import loss_case

ALGS = ('MC', 'TD', 'UPGO', 'VTRACE')
LOSS_KEYS = ('p', 'v', 'r', 'ent', 'total')


# ------------------------------------------------------------------ the float64 reference

def _log_selected(logits, action, emask):
    return torch.log_softmax(logits, dim=-1).gather(-1, action) * emask


def _scan(algorithm, v, returns, rewards, lmb, gamma, rho):
    """Targets and advantages of one head: v, rewards (B, T, P, 1), returns (B, 1 | T, P, 1), rho (B, T, Pp, 1).
    MC     target = returns
    TD     target[T-1] = returns[T-1];  target[t] = r[t] + gamma ((1 - lmb) v[t+1] + lmb target[t+1])
    UPGO   as TD with max(v[t+1], (1 - lmb) v[t+1] + lmb target[t+1])
    VTRACE delta[t] = rho[t] (r[t] + gamma v[t+1] - v[t]), v[T] = returns[T-1];
           acc[t] = delta[t] + gamma lmb rho[t] acc[t+1];  target = vs = acc + v;
           advantage[t] = r[t] + gamma vs[t+1] - v[t], vs[T] = returns[T-1]
    The advantage of the first three is target - v."""
    T = v.shape[1]
    r = rewards if rewards is not None else torch.zeros_like(v)
    last = returns[:, -1].expand_as(v[:, -1])
    if algorithm == 'MC':
        tgt = returns.expand_as(v)
        return tgt, tgt - v
    if algorithm in ('TD', 'UPGO'):
        rows = [None] * T
        rows[T - 1] = last
        for t in range(T - 2, -1, -1):
            mix = (1 - lmb) * v[:, t + 1] + lmb * rows[t + 1]
            if algorithm == 'UPGO':
                mix = torch.maximum(v[:, t + 1], mix)
            rows[t] = r[:, t] + gamma * mix
        tgt = torch.stack(rows, dim=1)
        return tgt, tgt - v
    if algorithm == 'VTRACE':
        rho = rho.expand_as(v)
        v_next = torch.cat([v[:, 1:], last.unsqueeze(1)], dim=1)
        delta = rho * (r + gamma * v_next - v)
        rows = [None] * T
        rows[T - 1] = delta[:, T - 1]
        for t in range(T - 2, -1, -1):
            rows[t] = delta[:, t] + gamma * lmb * rho[:, t] * rows[t + 1]
        vs = torch.stack(rows, dim=1) + v
        vs_next = torch.cat([vs[:, 1:], last.unsqueeze(1)], dim=1)
        return vs, r + gamma * vs_next - v
    raise ValueError('No algorithm named %s' % algorithm)


def reference_loss(outputs, batch, args):
    """(losses, dcnt, magnitudes): the losses as 0-d tensors with autograd through the target policy, the value
    head and the return head (targets, advantages and importance ratios are constants, train.py:228-232), dcnt a
    float, magnitudes[k] the sum of |terms| of losses[k]."""
    pol = outputs['policy']
    value, ret_out = outputs.get('value'), outputs.get('return')
    action, em = batch['action'], batch['episode_mask']
    tm, om = batch['turn_mask'], batch['observation_mask']

    lt = _log_selected(pol, action, em)
    lb = _log_selected(batch['policy'], action, em)
    rho = torch.exp(lt.detach() - lb).clamp(0, 1)            # clipped_rhos and cs are the same clamp

    lmb, gamma = args['lambda'], args['gamma']
    targets = {}
    adv = torch.zeros_like(tm)
    if value is not None:
        v = value.detach()
        if args['turn_based_training'] and v.shape[2] == 2:
            v = (v - v.flip(2)) / (om.sum(dim=2, keepdim=True) + 1e-8)
        v = v * em + batch['outcome'] * (1 - em)
        head = (v, batch['outcome'], None, lmb, 1.0, rho)
        targets['value'], a = _scan(args['value_target'], *head)
        if args['policy_target'] != args['value_target']:
            _, a = _scan(args['policy_target'], *head)
        adv = adv + a
    if ret_out is not None:
        head = (ret_out.detach(), batch['return'], batch['reward'], lmb, gamma, rho)
        targets['return'], a = _scan(args['value_target'], *head)
        if args['policy_target'] != args['value_target']:
            _, a = _scan(args['policy_target'], *head)
        adv = adv + a
    turn_adv = (rho * adv * tm).sum(dim=2, keepdim=True)     # (B, T, 1, 1)

    losses, mags = {}, {}
    terms = -lt * turn_adv
    losses['p'], mags['p'] = terms.sum(), terms.detach().abs().sum()
    base, base_mag = losses['p'], mags['p']
    if value is not None:
        terms = (value - targets['value']) ** 2 * om / 2
        losses['v'], mags['v'] = terms.sum(), terms.detach().abs().sum()
        base, base_mag = base + losses['v'], base_mag + mags['v']
    if ret_out is not None:
        x = ret_out - targets['return']
        terms = torch.where(x.abs() < 1, 0.5 * x * x, x.abs() - 0.5) * om
        losses['r'], mags['r'] = terms.sum(), terms.detach().abs().sum()
        base, base_mag = base + losses['r'], base_mag + mags['r']
    logp = torch.log_softmax(pol, dim=-1)
    plogp = torch.where(logp > -1e30, logp.exp() * logp, torch.zeros_like(logp))   # 0 log 0 = 0
    ent = -plogp.sum(-1) * tm.sum(-1)                         # (B, T, Pp) x (B, T, P)
    losses['ent'], mags['ent'] = ent.sum(), ent.detach().abs().sum()
    decayed = ent * (1 - batch['progress'] * (1 - args['entropy_regularization_decay']))
    coef = args['entropy_regularization']
    losses['total'] = base - coef * decayed.sum()
    mags['total'] = base_mag + abs(coef) * decayed.detach().abs().sum()
    return losses, float(tm.sum()), {k: float(m) for k, m in mags.items()}


# ------------------------------------------------------------------ the case generator

def make_case(B, T, P=2, Pp=1, A=9, heads=(True, True), vt='TD', pt='TD', lmb=0.7, gamma=0.8, tbt=True, seed=0):
    """One loss problem as float32 CPU tensors in the make_batch layout: {'outputs', 'batch', 'args', 'w', 'spec'}.

    Every case holds, as far as its size allows: episode tails of a different length per trajectory down to one
    live step, all-zero turn_mask rows on live steps, observation_mask zeros with at least one observer per live
    step, progress 0 and 1, the actions 0 and A - 1, -1e32 on the same non-chosen logits of both policies,
    importance ratios on both sides of the clip and return-head residuals on both sides of 1.  `w` weights the
    five losses (p, v, r, ent, total) for the backward: one entry is 0, at least one negative."""
    assert Pp in (1, P)
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * T + 31 * B + P)
    rand = lambda *s: torch.rand(*s, generator=g)        # noqa: E731
    randn = lambda *s: torch.randn(*s, generator=g)      # noqa: E731

    L = torch.randint(1, T + 1, (B,), generator=g)
    L[0] = 1
    if B > 1:
        L[1] = T
    if B > 2 and T > 2:
        L[2] = max(2, (T + 1) // 2)
    live = (torch.arange(T).view(1, T) < L.view(B, 1)).float()                    # (B, T)

    turn = torch.randint(0, P, (B, T), generator=g)
    seat = torch.nn.functional.one_hot(turn, P).float()                           # (B, T, P)
    tm = seat.clone()
    if Pp == P:
        tm = torch.maximum(tm, (rand(B, T, P) < 0.4).float())
    tm = tm * (rand(B, T, 1) >= 0.2).float()
    tm[B - 1, 0] = 0.0                                                            # a live step nobody moves at
    tm = tm * live.unsqueeze(-1)
    om = torch.maximum(seat, (rand(B, T, P) < 0.6).float()) * live.unsqueeze(-1)

    progress = rand(B, T, 1)
    progress.view(-1)[0] = 0.0
    progress.view(-1)[-1] = 1.0

    action = torch.randint(0, A, (B, T, Pp, 1), generator=g)
    action.view(-1)[-1] = A - 1
    action.view(-1)[0] = 0
    tpol = 1.5 * randn(B, T, Pp, A)
    bpol = tpol + 1.5 * randn(B, T, Pp, A)
    illegal = (rand(B, T, Pp, A) < 0.3).scatter(-1, action, False)
    tpol = tpol.masked_fill(illegal, -1e32)
    bpol = bpol.masked_fill(illegal, -1e32)

    outputs = {'policy': tpol}
    if heads[0]:
        outputs['value'] = torch.tanh(randn(B, T, P, 1))
    if heads[1]:
        outputs['return'] = 1.5 * randn(B, T, P, 1)
    batch = {
        'policy': bpol, 'action': action, 'outcome': 2 * rand(B, 1, P, 1) - 1,
        'reward': 0.5 * randn(B, T, P, 1), 'return': randn(B, T, P, 1),
        'episode_mask': live.view(B, T, 1, 1).contiguous(), 'turn_mask': tm.unsqueeze(-1).contiguous(),
        'observation_mask': om.unsqueeze(-1).contiguous(), 'progress': progress,
    }
    args = {'turn_based_training': tbt, 'observation': Pp == P and P > 1, 'forward_steps': T, 'lambda': lmb,
            'gamma': gamma, 'value_target': vt, 'policy_target': pt,
            'entropy_regularization': (0.1, 0.25)[seed % 2], 'entropy_regularization_decay': (0.1, 0.3)[seed // 2 % 2]}
    w = randn(5)
    w[seed % 5] = 0.0
    w[(seed + 1) % 5] = -w[(seed + 1) % 5].abs() - 0.25
    spec = dict(B=B, T=T, P=P, Pp=Pp, A=A, heads=tuple(heads), vt=vt, pt=pt, lmb=lmb, gamma=gamma, tbt=tbt, seed=seed)
    return {'outputs': outputs, 'batch': batch, 'args': args, 'w': w, 'spec': spec}


def objective(losses, w):
    """sum_k w_k losses[k] over the losses present, k in the order p, v, r, ent, total."""
    return sum(w[i] * losses[k] for i, k in enumerate(LOSS_KEYS) if k in losses)


def _cast(t, dtype):
    return t.to(dtype) if t.is_floating_point() else t


def evaluate(fn, case, dtype=torch.float32, device=None):
    """fn(outputs, batch, args) on the case's tensors as leaves of `dtype`; returns
    {'losses': {k: float}, 'dcnt': float, 'grads': {head: float64 CPU tensor}, 'extra': what fn returned beyond
    (losses, dcnt)} with the gradients of objective(losses, w)."""
    put = lambda t: _cast(t, dtype) if device is None else _cast(t, dtype).to(device)   # noqa: E731
    leaves = {k: put(t).requires_grad_(True) for k, t in case['outputs'].items()}
    batch = {k: put(t) for k, t in case['batch'].items()}
    out = fn(leaves, batch, case['args'])
    losses, dcnt = out[0], out[1]
    names = list(leaves)
    grads = torch.autograd.grad(objective(losses, put(case['w'])), [leaves[k] for k in names],
                                allow_unused=True)
    return {'losses': {k: float(v.detach()) for k, v in losses.items()}, 'dcnt': float(dcnt),
            'grads': {k: (torch.zeros_like(leaves[k]) if g is None else g).detach().double().cpu()
                      for k, g in zip(names, grads)},
            'extra': out[2:]}


def reference64(case):
    """The float64 reference's losses, gradients and per-loss magnitudes ('mags') on a case."""
    r = evaluate(reference_loss, case, torch.float64)
    r['mags'] = r.pop('extra')[0]
    return r


def oracle32(case):
    """The float32 CPU oracle (the reference project's arithmetic) on a case."""
    return evaluate(ol.loss_from_outputs, case, torch.float32)


def error_ratios(got, ref):
    """{quantity: (error, scale)} of a float32 result against reference64's: for a loss |difference| and the sum
    of |terms|; for a gradient tensor the largest |difference| and the largest |reference|."""
    out = {}
    for k, v in ref['losses'].items():
        out[k] = (abs(got['losses'][k] - v), ref['mags'][k])
    for k, gr in ref['grads'].items():
        out['d' + k] = (float((got['grads'][k] - gr).abs().max()), float(gr.abs().max()))
    return out


# ------------------------------------------------------------------ the tests of the reference itself

def _rel(a, b, rel):
    return abs(a - b) <= rel * abs(b)


def test_reference_on_recorded_losses(golden_loss):
    """tests/golden/loss.*: the reference project's own losses and gradients w.r.t. the raw network outputs."""
    meta, arrays = golden_loss
    assert len(meta) >= 7
    for c in meta:
        batch, net = loss_case(arrays, c)
        batch = {k: _cast(t, torch.float64) for k, t in batch.items()}
        net = net.double()
        outputs = ol.forward_prediction(net, None, batch, c['args'])
        assert outputs['policy'].dtype == torch.float64
        losses, dcnt, mags = reference_loss(outputs, batch, c['args'])
        assert dcnt == c['dcnt']
        assert set(losses) == set(c['losses'])
        for k, v in c['losses'].items():
            assert _rel(losses[k].item(), v, 1e-6), (c['name'], k, losses[k].item(), v)
            assert mags[k] >= abs(losses[k].item()) * (1 - 1e-12)
        losses['total'].backward()
        pre = '%d:' % c['id']
        np.testing.assert_allclose(net.p.grad.numpy(), arrays[pre + 'grad.policy'], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(net.v.grad.numpy(), arrays[pre + 'grad.value'], rtol=1e-5, atol=1e-6)
        if c['has_return']:
            np.testing.assert_allclose(net.r.grad.numpy(), arrays[pre + 'grad.return'], rtol=1e-5, atol=1e-6)


# P, Pp, heads, (value_target, policy_target), lambda, gamma: every P with both Pp, every head combination,
# every algorithm on either side
GENERATED = [
    (1, 1, (True, True), ('TD', 'TD'), 0.7, 0.8),
    (1, 1, (False, True), ('VTRACE', 'MC'), 1.0, 1.0),
    (2, 1, (True, True), ('VTRACE', 'UPGO'), 0.7, 0.8),
    (2, 2, (True, False), ('MC', 'VTRACE'), 0.0, 0.8),
    (2, 1, (False, False), ('UPGO', 'UPGO'), 0.7, 1.0),
    (2, 2, (False, True), ('TD', 'UPGO'), 1.0, 0.8),
    (3, 1, (True, True), ('UPGO', 'TD'), 0.7, 0.8),
    (3, 3, (True, True), ('MC', 'MC'), 0.7, 1.0),
    (3, 3, (False, True), ('VTRACE', 'VTRACE'), 0.0, 0.8),
    (8, 1, (True, False), ('TD', 'MC'), 1.0, 0.8),
    (8, 8, (True, True), ('UPGO', 'VTRACE'), 0.7, 0.8),
    (8, 8, (False, False), ('MC', 'TD'), 0.7, 1.0),
    (2, 1, (True, True), ('TD', 'VTRACE'), 0.7, 0.8),
]


def _generated_case(i):
    P, Pp, heads, (vt, pt), lmb, gamma = GENERATED[i]
    return make_case(B=4, T=19, P=P, Pp=Pp, A=(9, 6, 70)[i % 3], heads=heads, vt=vt, pt=pt, lmb=lmb, gamma=gamma,
                     tbt=i != 12, seed=i)


def test_generated_cases_span_the_operator():
    assert {c[0] for c in GENERATED} == {1, 2, 3, 8}
    assert {(c[0], c[1]) for c in GENERATED} >= {(p, q) for p in (2, 3, 8) for q in (1, p)}
    assert {c[2] for c in GENERATED} == {(a, b) for a in (True, False) for b in (True, False)}
    assert {c[3][0] for c in GENERATED} == set(ALGS) and {c[3][1] for c in GENERATED} == set(ALGS)
    assert len(GENERATED) >= 12


@pytest.mark.parametrize('i', range(len(GENERATED)))
def test_reference_agrees_with_fp32_oracle(i):
    case = _generated_case(i)
    ref, got = reference64(case), oracle32(case)
    assert got['dcnt'] == ref['dcnt'] == float(case['batch']['turn_mask'].sum())
    assert set(got['losses']) == set(ref['losses'])
    for k, v in ref['losses'].items():
        assert _rel(got['losses'][k], v, 1e-6), (k, got['losses'][k], v)
    for k, gr in ref['grads'].items():
        np.testing.assert_allclose(got['grads'][k].numpy(), gr.numpy(), rtol=1e-5, atol=1e-6, err_msg=k)


@pytest.mark.parametrize('i', range(len(GENERATED)))
def test_generator_holds_every_edge(i):
    """What make_case promises, on cases of B = 4, T = 19 (large enough for all of it)."""
    case = _generated_case(i)
    s, b, o = case['spec'], case['batch'], case['outputs']
    B, T, P, Pp, A = s['B'], s['T'], s['P'], s['Pp'], s['A']
    em, tm, om = b['episode_mask'], b['turn_mask'], b['observation_mask']
    lengths = em.view(B, T).sum(1)
    assert lengths.min() == 1 and lengths.max() == T and len(set(lengths.tolist())) >= 3
    assert bool((em.view(B, T)[:, 1:] <= em.view(B, T)[:, :-1]).all())          # a tail, not holes
    live = em.view(B, T) > 0
    assert bool((tm.view(B, T, P).sum(-1)[live] == 0).any())
    assert bool((om.view(B, T, P).sum(-1)[live] >= 1).all())
    assert P == 1 or bool((om.view(B, T, P)[live] == 0).any())
    assert bool((tm[~live] == 0).all()) and bool((om[~live] == 0).all())
    assert b['progress'].min() == 0 and b['progress'].max() == 1
    act = b['action']
    assert act.min() == 0 and act.max() == A - 1 and act.dtype == torch.int64
    for pol in (o['policy'], b['policy']):
        assert bool((pol == -1e32).any())
        assert bool((pol.gather(-1, act) > -1e30).all())
    lt = _log_selected(o['policy'], act, em)
    lb = _log_selected(b['policy'], act, em)
    rho = torch.exp(lt - lb)[live]
    assert bool((rho < 1).any()) and bool((rho > 1).any())
    if 'return' in o:
        x = (o['return'] - b['return']).abs()
        assert bool((x < 1).any()) and bool((x > 1).any())
    w = case['w']
    assert int((w == 0).sum()) == 1 and bool((w < 0).any())
