"""The C51 head kernels (csrc/kernels/rainbow.hip: c51_train_kernel, c51_infer_kernel, c51_softmax)
and the stand-alone td_loss_c51_kernel (csrc/kernels/td_loss.hip) against a float64 reference of
the same operation, at the shapes where the kernels change path.

The head binding takes the logits rows as pointers, so the kernels run on synthetic fp32 logits
with no network: rows of ``KD`` floats = [A * atoms logits | pad | dueling value logits at VO | pad]
(VO = A * atoms rounded up to 32). The input pads hold 1e9: a kernel that read one would show it.

Reference (numpy float64, on the fp32 input values; nothing from ``models/losses.py``): dueling
combine per atom, softmax, Q = sum p z, argmax of the selection instance (first maximum wins,
an explicit loop), the projection in closed form
``m_i = sum_j p_j clip(1 - |clamp(r + g z_j) - z_i| / dz, 0, 1)``, cross-entropy, and
dL/dlogits = w / B (p - m) (dueling: advantage columns times (i == a) - 1 / A, value columns plain).

Cases: action counts on both sides of every template instance (AM = 4, 8, 18, 32); atoms 2, 21,
32 (VO == NO), 33, 51, 64; B = 1, 8, 9, 24 and 513 (the block-stride loop); plain / dueling, with
and without the Double-DQN instance; weights absent, random, containing an exact 0; the supports
(-10, 10), (0, 200, 21) and two whose fp32 ``(v_max - v_min) / dz`` rounds above N - 1. Every batch
starts with the projection's edge rows; row 8 has its logits scaled by 30, row 9 has two actions
with bit-identical selection logits (Double DQN cases).

Bounds. ``prio`` and the loss: rtol 1e-4, atol 1e-5 (test_kernels_gpu.py::test_td_loss_c51_kernel,
the same __expf / __logf arithmetic). ``dout16`` elementwise: |err| <= ulp |ref| + t, ulp = 2^-8
(bf16), 2^-11 (fp16), 0 (fp32), t = (1e-4 |g| + 1e-6) w_b / B with g the element before the
w_b / B factor ((p - m), times the dueling coefficient), all times the fp16 build's loss scale.
A row whose two largest selection Q values lie within 1e-4 (v_max - v_min) in the reference is
left out (fp32 cannot be asked to pick float64's action there; the exact tie is not such a row);
at most one row in 16, asserted per case on the reference alone. The loss reference takes the
kernel's own priority for such a row.

Largest observed err / bound over all cases of the build (one MI355X run): bf16 0.969 (the
storage rounding: round-to-nearest reaches 2^-8 at the bottom of a binade), fp16 0.767, fp32 0.300.
Before the kernels placed a target clamped to v_max on the last atom exactly, the bf16 case
(B 24, A 19, atoms 64) missed the bound on the row scaled by 30: fp32 ``(v_max - v_min) / dz`` is
62.999996 there, so 3.8e-6 of a near one-hot target's mass went to atom 62 (err 8.7e-8 against a
bound of about 5e-8). The 126,336-byte inference launch runs without a
hipFuncAttributeMaxDynamicSharedMemorySize call.
"""
import numpy as np
import pytest
import torch

import head_ref as hr
from head_ref import DEV, HID, PAD_IN, dims as _dims, ext as _ext

pytestmark = pytest.mark.gpu
FN = 'qnet_c51_head'
S10 = (-10.0, 10.0)


def _blocks(B):
    return min((B + 7) // 8, 64)   # eight samples (one per wave) per learner block


# ------------------------------------------------------------------ inputs (CPU, seeded)
def _inputs(B, A, N, dueling, double, wmode, sup, seed):
    v_min, v_max = sup
    g = torch.Generator().manual_seed(seed)
    NO, VO, KD = _dims(A, N, dueling)
    dz = (v_max - v_min) / (N - 1)
    zf = torch.linspace(v_min, v_max, N)
    x = torch.randn(3, B, A, N, generator=g)
    v = torch.randn(3, B, N, generator=g)
    tie = None
    if B > 8:
        x[:, 8] *= 30.0
        v[:, 8] *= 30.0
    if B > 9 and double:
        # two actions of the selection instance bit-identical and (tilted to the high atoms) the
        # greedy ones; the target's rows of the two differ, so the later maximum shows
        i1, i2 = A // 3, A - 1
        x[2, 9, i1] += 3.0 * torch.linspace(-1.0, 1.0, N)
        x[2, 9, i2] = x[2, 9, i1]
        tie = (9, i1, i2)
    # (reward, done, gamma) of the edge rows
    edges = [(v_max + 1.0, 1.0, 0.99), (v_min - 1.0, 1.0, 0.99), (v_max, 1.0, 0.99), (0.0, 1.0, 0.99),
             (float(zf[N // 3]), 1.0, 0.99), (0.0, 0.0, 1.0), (dz / 2, 0.0, 1.0),
             (v_min + 0.3 * (v_max - v_min), 0.0, 0.0)]
    rew, done, gam = hr.draw_transitions(g, B, edges, (v_max - v_min) / 4)
    act = hr.draw_actions(g, B, A)
    wts, zrow = hr.draw_weights(g, B, wmode)
    rows = torch.full((3, B, KD), PAD_IN)
    rows[:, :, :NO] = x.reshape(3, B, NO)
    if dueling:
        rows[:, :, VO:VO + N] = v
    return dict(B=B, A=A, N=N, dueling=dueling, double=double, sup=sup, rows=rows.float(), rew=rew, done=done,
                gam=gam, act=act, wts=wts, tie=tie, zrow=zrow)


# ------------------------------------------------------------------ float64 reference
def _dist64(rows, A, N, dueling):
    """Probabilities [.., A, N] and Q [.., A] of logits rows [.., KD]."""
    NO, VO, _ = _dims(A, N, dueling)
    r = rows.double().numpy()
    x = r[..., :NO].reshape(r.shape[:-1] + (A, N))
    if dueling:
        x = x + r[..., None, VO:VO + N] - x.mean(-2, keepdims=True)
    x = x - x.max(-1, keepdims=True)
    e = np.exp(x)
    return x, e / e.sum(-1, keepdims=True)


def _support(sup, N):
    return np.linspace(sup[0], sup[1], N), (sup[1] - sup[0]) / (N - 1)


def _reference(c):
    B, A, N, sup = c['B'], c['A'], c['N'], c['sup']
    z, dz = _support(sup, N)
    x, p = _dist64(c['rows'], A, N, c['dueling'])            # [3, B, A, N] (x: max-subtracted logits)
    q = (p * z).sum(-1)                                       # [3, B, A]
    qs = q[2 if c['double'] else 1]
    best = np.zeros(B, dtype=np.int64)
    for b in range(B):
        for i in range(1, A):
            if qs[b, i] > qs[b, best[b]]:                     # strictly greater: the first maximum wins
                best[b] = i
    top = np.sort(qs, axis=1)
    skip = (top[:, -1] - top[:, -2]) < 1e-4 * (sup[1] - sup[0])
    if c['tie'] is not None:
        b, i1, i2 = c['tie']
        assert qs[b, i1] == qs[b, i2] == qs[b].max() and best[b] == i1
        skip[b] = False
    pt = p[1][np.arange(B), best]                             # [B, N]
    r, d, gm = (c[k].double().numpy() for k in ('rew', 'done', 'gam'))
    tz = np.clip(r[:, None] + (gm * (1.0 - d))[:, None] * z[None, :], sup[0], sup[1])
    m = (pt[:, :, None] * np.clip(1.0 - np.abs(tz[:, :, None] - z[None, None, :]) / dz, 0.0, 1.0)).sum(1)
    act = c['act'].long().numpy()
    xo = x[0][np.arange(B), act]
    logp = xo - np.log(np.exp(xo).sum(-1, keepdims=True))
    ce = -(m * logp).sum(-1)
    w = np.ones(B) if c['wts'] is None else c['wts'].double().numpy()
    g = p[0][np.arange(B), act] - m                           # [B, N]: dL/dlogits before w / B
    return dict(q=q, best=best, skip=skip, m=m, ce=ce, w=w, g=g)


def _dout_ref(c, ref):
    """(g [B, KD] before the w / B factor, written-column mask [KD])."""
    B, A, N = c['B'], c['A'], c['N']
    NO, VO, KD = _dims(A, N, c['dueling'])
    g = np.zeros((B, KD))
    onehot = np.eye(A)[c['act'].long().numpy()]               # [B, A]
    coef = onehot - (1.0 / A if c['dueling'] else 0.0)
    g[:, :NO] = (coef[:, :, None] * ref['g'][:, None, :]).reshape(B, NO)
    mask = np.zeros(KD, dtype=bool)
    mask[:NO] = True
    if c['dueling']:
        g[:, VO:VO + N] = ref['g']
        mask[VO:VO + N] = True
    return g, mask


# ------------------------------------------------------------------ launches
_ratios = {}


def _check_train(variant, c):
    ref = _reference(c)
    g, mask = _dout_ref(c, ref)
    call = FN, [c['B'], c['A'], HID, int(c['dueling']), 0, 0], [c['N']], [c['sup'][0], c['sup'][1]]
    # (priorities: the unweighted cross-entropy, which is the per-sample loss too)
    hr.check_train(variant, c, call, 3 if c['double'] else 2, mask.size, _blocks(c['B']),
                   dict(g=g, t=1e-4 * np.abs(g) + 1e-6, mask=mask, prio=ref['ce'], per=ref['ce'], w=ref['w'],
                        skip=ref['skip']), ('ce', 'ce', 'a logits / value column'), _ratios)


TRAIN_CASES = [
    # B, A, atoms, dueling, double, weights, support
    (24, 2, 51, 0, 0, 'none', S10), (24, 4, 51, 1, 1, 'rand', S10), (24, 5, 51, 0, 1, 'zero', S10),
    (24, 8, 51, 1, 0, 'rand', S10), (24, 9, 51, 1, 1, 'none', S10), (24, 18, 51, 1, 1, 'zero', S10),
    (24, 19, 51, 0, 1, 'rand', S10),                                               # AM boundaries
    (24, 6, 2, 1, 1, 'rand', S10), (24, 6, 21, 1, 0, 'none', S10),                 # under one 32-column tile
    (24, 4, 32, 1, 1, 'rand', S10), (24, 5, 32, 0, 0, 'zero', S10), (24, 18, 32, 1, 1, 'none', S10),   # VO == NO
    (24, 6, 33, 1, 1, 'rand', S10), (24, 6, 64, 1, 1, 'zero', S10), (24, 19, 64, 0, 0, 'rand', S10),
    (1, 6, 51, 1, 1, 'zero', S10), (8, 6, 51, 0, 1, 'rand', S10), (9, 6, 51, 1, 0, 'none', S10),
    (513, 6, 51, 1, 1, 'zero', S10),                                               # the block-stride loop
    (24, 6, 21, 0, 1, 'rand', (0.0, 200.0)), (24, 6, 62, 1, 1, 'rand', (-1.0, 1.0)),
    (24, 4, 30, 0, 0, 'none', (-21.0, 21.0)),
]
OTHER_BUILDS_CASE = (24, 6, 51, 1, 1, 'zero', S10)


def _seed(B, A, N, dueling, double):
    if N == 2:      # (two atoms: the row scaled by 30 is always a near-tie; this seed has no second one)
        return 1
    return 1000 * A + 10 * N + B + 2 * dueling + double


def _make(case):
    B, A, N, dueling, double, wmode, sup = case
    return _inputs(B, A, N, dueling, double, wmode, sup, _seed(B, A, N, dueling, double))


@pytest.mark.parametrize('B,A,N,dueling,double,wmode,sup', TRAIN_CASES)
def test_c51_train_matches_float64(B, A, N, dueling, double, wmode, sup):
    _check_train('', _make((B, A, N, dueling, double, wmode, sup)))


@pytest.mark.parametrize('variant', ['f16', 'f32'])
def test_c51_train_other_builds(variant):
    _check_train(variant, _make(OTHER_BUILDS_CASE))


# ------------------------------------------------------------------ inference kernel
def _infer(rows, B, A, N, dueling, sup):
    return hr.infer(_ext(''), FN, [N], [sup[0], sup[1]], rows, B, A, dueling)


INFER_POINTS = [(2, 51, 0), (4, 51, 1), (5, 51, 0), (8, 51, 1), (9, 51, 1), (18, 51, 1), (19, 51, 0),
                (6, 2, 1), (6, 21, 1), (4, 32, 1), (5, 32, 0), (6, 33, 1), (6, 64, 1), (18, 64, 0)]


@pytest.mark.parametrize('B', [1, 32])
@pytest.mark.parametrize('A,N,dueling', INFER_POINTS)
def test_c51_infer_matches_float64(A, N, dueling, B):
    """q_values' kernel; B = 32 with 18 actions of 51 atoms takes 126,336 bytes of dynamic LDS."""
    c = _inputs(B, A, N, dueling, False, 'none', S10, _seed(B, A, N, dueling, 0))
    q = _infer(c['rows'][0], B, A, N, dueling, S10)
    _, p = _dist64(c['rows'][0], A, N, dueling)
    ref = (p * _support(S10, N)[0]).sum(-1)
    np.testing.assert_allclose(q, ref, rtol=1e-4, atol=1e-5 * 10.0)


def test_c51_infer_other_support():
    B, A, N, sup = 32, 6, 62, (-1.0, 1.0)
    c = _inputs(B, A, N, 1, False, 'none', sup, 7)
    q = _infer(c['rows'][0], B, A, N, 1, sup)
    _, p = _dist64(c['rows'][0], A, N, 1)
    ref = (p * _support(sup, N)[0]).sum(-1)
    np.testing.assert_allclose(q, ref, rtol=1e-4, atol=1e-5 * 1.0)


def test_c51_infer_refuses_rows_beyond_lds():
    """64 rows of 18 x 51 logits are 252,672 bytes: refused before any launch."""
    B, A, N = 64, 18, 51
    r = torch.zeros(B, _dims(A, N, 0)[2], device=DEV)
    q = torch.full((B * A,), float('nan'), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match='too large'):
        _ext('').qnet_c51_head([B, A, HID, 0, 0, 1], [N], [-10.0, 10.0], [], [], [], [], [],
                               [0] * 7 + [q.data_ptr()] + [0] * 5, [], [], [], [], [], 0, [r.data_ptr()], 0, [])
    torch.cuda.synchronize()
    assert torch.isnan(q).all()


# ------------------------------------------------------------------ stand-alone td_loss_c51 (the MLP path)
@pytest.mark.parametrize('N,sup', [(51, S10), (64, S10), (62, (-1.0, 1.0))])
def test_td_loss_c51_matches_float64(N, sup):
    """ops/td.py's kernel on the same edge rows; tolerances of test_td_loss_c51_kernel."""
    from dist_dqn_amd.ops.td import td_loss
    B, A = 24, 4
    c = _inputs(B, A, N, 0, True, 'rand', sup, 50 + N)
    ref = _reference(c)
    assert not ref['skip'].any(), 'near-ties in the reference: pick another seed'
    x = c['rows'][:, :, :A * N].reshape(3, B, A, N).to(DEV)
    xg = x[0].clone().requires_grad_(True)
    loss, prio = td_loss(xg, c['act'].to(DEV), c['rew'].to(DEV), c['done'].to(DEV), c['gam'].to(DEV), x[1], x[2],
                         c['wts'].to(DEV), distributional=True, v_min=sup[0], v_max=sup[1])
    loss.backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(prio.cpu().double().numpy(), ref['ce'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(float(loss.detach()), float((ref['w'] * ref['ce']).sum() / B), rtol=1e-4, atol=1e-5)
    g, _ = _dout_ref(c, ref)
    want = (g[:, :A * N] * (ref['w'] / B)[:, None]).reshape(B, A, N)
    np.testing.assert_allclose(xg.grad.cpu().double().numpy(), want, rtol=1e-4, atol=1e-6)
