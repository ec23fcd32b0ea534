"""The wide QR-DQN head kernels (csrc/kernels/qr_wide_head.hip: qr_wide_train_kernel,
qr_wide_infer_kernel; 64 < N <= 256 quantiles, N % 4 == 0) against a float64 reference of the same
operation, at the shapes where the kernels change path.

The method, the inputs, the reference and the bounds are those of test_qr_head_gpu.py (whose
helpers this file imports): synthetic fp32 rows ``KD`` = [A * N quantiles | pad | dueling value
quantiles at VO | pad] with 1e9 in the input pads, sentinel-filled outputs, a numpy float64
reference, two launches bit-equal, no pad column and no row beyond ``B`` written, every real
column written.

Cases: N = 68 and 72 (the smallest wide counts: two waves, the second with 4 / 8 threads and a
partial last lane group of the 16-byte loads), 128 / 132 (two full waves / a third wave of four
threads), 200 (the paper's count: four waves, the last with 8 threads), 252 / 256 (the last lane
of the streaming layout partial / every lane and thread in use); action counts at, just above
and well above the wave count (A = 2 on two waves; 4, 5, 6; 18 / 19 and 32: more than one
four-action load batch per wave); B = 1, 8, 9, 24, 32 and, more samples than the 64 learner blocks take at
once, 130 and 513; plain / dueling, with and without the Double-DQN instance; weights absent,
random, containing an exact 0; kappa 1 and 0.5.

Bounds (test_qr_head_gpu.py's docstring derives them). ``prio`` and the loss: rtol 1e-4, atol
1e-5. ``dout16`` elementwise: |err| <= ulp |ref| + t_g |coef| w_b / B times the fp16 build's loss
scale, t_g = ((2 (A + 2) + 2) or 2) e M / kappa + (N + 4) e: the (N + 4) e term holds for any
order of an N-term sum of terms <= 1, so the four accumulator chains of the pairwise loop and the
per-wave partials of the dueling action mean stay inside it. Near-tie rows are left out, at most
one row in 16, asserted per case on the reference alone and in a test that needs no GPU.
Q of the inference kernel: (3 N + A + 4) e M with dueling, (N + 2) e M plain.

Largest observed err / bound over all cases of the build (one MI355X run): bf16 0.993 and fp16
0.938 (the storage rounding reaches its full step at the bottom of a binade), fp32 0.042; Q of the
inference kernel 0.004. Largest |err| of ``prio`` seen 1.7e-4 at values up to 3.1e3.
"""
import numpy as np
import pytest
import torch

from test_qr_head_gpu import (BUILDS, DEV, E24, HID, SENT, _dims, _dout_ref, _inputs, _quantiles64, _reference, _seed,
                              _t_g)

TRAIN_CASES = [
    # B, A, N, dueling, double, weights, kappa
    (24, 2, 68, 0, 0, 'none', 1.0), (24, 6, 68, 1, 1, 'rand', 1.0), (24, 6, 72, 1, 0, 'zero', 0.5),
    (24, 4, 128, 1, 1, 'rand', 1.0), (24, 5, 128, 0, 1, 'zero', 1.0), (24, 6, 132, 1, 1, 'none', 0.5),
    (24, 6, 200, 1, 1, 'zero', 1.0), (32, 18, 200, 1, 1, 'rand', 1.0), (24, 19, 200, 0, 1, 'none', 1.0),
    (24, 32, 200, 1, 0, 'rand', 0.5),
    (24, 6, 252, 1, 1, 'rand', 1.0), (24, 6, 256, 1, 1, 'zero', 1.0), (24, 18, 256, 0, 0, 'rand', 1.0),
    (1, 6, 200, 1, 1, 'zero', 1.0), (8, 6, 200, 0, 1, 'rand', 1.0), (9, 6, 200, 1, 0, 'none', 1.0),
    (513, 6, 68, 1, 1, 'zero', 1.0), (130, 6, 200, 1, 1, 'rand', 1.0),      # more samples than learner blocks
]
OTHER_BUILDS_CASE = (24, 6, 200, 1, 1, 'zero', 1.0)
INFER_POINTS = [(2, 68, 0), (6, 72, 1), (5, 128, 0), (18, 200, 1), (19, 200, 0), (6, 252, 1), (18, 256, 0)]


def _blocks(B):
    return min(B, 64)              # one sample per learner block at a time


def _make(case):
    B, A, N, dueling, double, wmode, kappa = case
    return _inputs(B, A, N, dueling, double, wmode, kappa, _seed(B, A, N, dueling, double))


_cache = {}


def _case(case):
    """(inputs, float64 reference) of a case: computed once, shared, never modified."""
    if case not in _cache:
        c = _make(case)
        _cache[case] = (c, _reference(c))
    return _cache[case]


def _ext(variant):
    from dist_dqn_amd.ops import _ext as loader
    return loader.load(required=True, variant=variant)


def _train(ext, c, act_t):
    B, A, N = c['B'], c['A'], c['N']
    _, _, KD = _dims(A, N, c['dueling'])
    t = {k: c[k].to(DEV).contiguous() for k in ('rows', 'rew', 'done', 'gam', 'act')}
    wts = None if c['wts'] is None else c['wts'].to(DEV)
    dout = torch.full(((B + 8) * KD,), SENT, dtype=act_t, device=DEV)
    prio = torch.full((B + 8,), SENT, dtype=torch.float32, device=DEV)
    parts = torch.full((72,), SENT, dtype=torch.float32, device=DEV)
    io = [t['act'].data_ptr(), t['rew'].data_ptr(), t['done'].data_ptr(), t['gam'].data_ptr(),
          0 if wts is None else wts.data_ptr(), 0, prio.data_ptr()] + [0] * 6
    lg = [t['rows'][i].data_ptr() for i in range(3 if c['double'] else 2)]
    ext.qnet_qr_wide_head([B, A, HID, int(c['dueling']), 0, 0], [N], [float(c['kappa'])], [], [], [], [], [], io,
                          [], [], [], [], [], lg, 0, [parts.data_ptr(), dout.data_ptr()])
    torch.cuda.synchronize()
    return dout.cpu(), prio.cpu(), parts.cpu()


_ratios = {}


def _check_train(variant, case):
    act_t, ulp, scale = BUILDS[variant]
    c, ref = _case(case)
    B, A, N = c['B'], c['A'], c['N']
    NO, VO, KD = _dims(A, N, c['dueling'])
    skip = ref['skip']
    assert int(skip.sum()) * 16 <= B, ('near-ties in the reference: pick another seed', np.nonzero(skip)[0])
    keep = ~skip
    ext = _ext(variant)
    dout, prio, parts = _train(ext, c, act_t)
    dout2, prio2, parts2 = _train(ext, c, act_t)
    assert torch.equal(prio, prio2) and torch.equal(dout.view(torch.uint8), dout2.view(torch.uint8)), 'repeatability'
    assert torch.equal(parts, parts2), 'repeatability of the loss partials'
    # layout and write coverage
    d = dout.double().view(B + 8, KD).numpy()
    g, cf, mask = _dout_ref(c, ref)
    assert (d[:B][:, ~mask] == SENT).all(), 'a pad column was written'
    assert (d[B:] == SENT).all() and (prio[B:] == SENT).all(), 'a row beyond B was written'
    assert (d[:B][:, mask] != SENT).all() and (prio[:B] != SENT).all(), 'a quantile / value column was left unwritten'
    nb = _blocks(B)
    assert (parts[nb:] == SENT).all() and (parts[:nb] != SENT).all(), 'loss partials'
    # priorities (the unweighted per-sample loss) and the loss (the fc dgrad launch's aux duty: sum / B)
    pk = prio[:B].double().numpy()
    print('per: max |err| %.3g at |per| up to %.3g' % (np.abs(pk - ref['per'])[keep].max(), ref['per'].max()))
    np.testing.assert_allclose(pk[keep], ref['per'][keep], rtol=1e-4, atol=1e-5)
    loss_ref = float((ref['w'] * np.where(keep, ref['per'], pk)).sum() / B)
    np.testing.assert_allclose(float(parts[:nb].double().sum()) / B, loss_ref, rtol=1e-4, atol=1e-5)
    # dL/dtheta rows
    wb = (ref['w'] / B)[:, None]
    want = g * wb * scale
    bound = ulp * np.abs(want) + _t_g(c, ref)[:, None] * cf * wb * scale
    err = np.abs(d[:B] - want)
    sel = keep[:, None] & mask[None, :]
    ratio = np.where(sel & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0)
    _ratios[variant] = max(_ratios.get(variant, 0.0), float(ratio.max()))
    print('dout16 %r: max err / bound %.3f (build so far %.3f)' % (variant, ratio.max(), _ratios[variant]))
    bad = sel & (err > bound)
    assert not bad.any(), (int(bad.sum()), [(int(b), int(k), d[b, k], want[b, k]) for b, k in np.argwhere(bad)[:5]])
    if c['zrow'] is not None:
        assert (d[c['zrow']][mask] == 0.0).all(), 'zero-weight row'


def test_seeded_cases_stay_within_the_near_tie_cap():
    """No GPU: the reference alone, for every case this file launches."""
    for case in TRAIN_CASES + [OTHER_BUILDS_CASE]:
        c, ref = _case(case)
        assert int(ref['skip'].sum()) * 16 <= c['B'], (case, np.nonzero(ref['skip'])[0])
        assert c['tie'] is None or not ref['skip'][c['tie'][0]]
        assert (ref['per'] >= 0).all() and (np.abs(ref['g']) <= 1.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize('B,A,N,dueling,double,wmode,kappa', TRAIN_CASES)
def test_qr_wide_train_matches_float64(B, A, N, dueling, double, wmode, kappa):
    _check_train('', (B, A, N, dueling, double, wmode, kappa))


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['f16', 'f32'])
def test_qr_wide_train_other_builds(variant):
    _check_train(variant, OTHER_BUILDS_CASE)


@pytest.mark.gpu
def test_qr_wide_head_refuses_bad_arguments():
    """Quantile count and kappa are checked before any launch: the output buffer stays untouched."""
    ext = _ext('')
    r = torch.zeros(4, _dims(6, 260, 0)[2], device=DEV)
    q = torch.full((4 * 6,), float('nan'), dtype=torch.float32, device=DEV)
    io = [0] * 7 + [q.data_ptr()] + [0] * 5
    for n, kappa, word in ((64, 1.0, 'quantiles'), (66, 1.0, 'quantiles'), (260, 1.0, 'quantiles'), (200, 0.0, 'kappa')):
        with pytest.raises(RuntimeError, match=word):
            ext.qnet_qr_wide_head([4, 6, HID, 0, 0, 1], [n], [kappa], [], [], [], [], [], io, [], [], [], [], [],
                                  [r.data_ptr()], 0, [])
    torch.cuda.synchronize()
    assert torch.isnan(q).all()


# ------------------------------------------------------------------ inference kernel
def _infer(ext, rows, B, A, N, dueling):
    r = rows.to(DEV).contiguous()
    q = torch.full((B * A + 8,), float('nan'), dtype=torch.float32, device=DEV)
    ext.qnet_qr_wide_head([B, A, HID, int(dueling), 0, 1], [N], [1.0], [], [], [], [], [],
                          [0] * 7 + [q.data_ptr()] + [0] * 5, [], [], [], [], [], [r.data_ptr()], 0, [])
    torch.cuda.synchronize()
    return q.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize('B', [1, 32, 513])
@pytest.mark.parametrize('A,N,dueling', INFER_POINTS)
def test_qr_wide_infer_matches_float64(A, N, dueling, B):
    """q_values' kernel: Q = mean over quantiles."""
    c = _inputs(B, A, N, dueling, False, 'none', 1.0, _seed(B, A, N, dueling, 0))
    q = _infer(_ext(''), c['rows'][0], B, A, N, dueling)
    assert torch.isnan(q[B * A:]).all(), 'written beyond [B][A]'
    assert not torch.isnan(q[:B * A]).any(), 'q_out left unwritten'
    th, mag = _quantiles64(c['rows'][0], A, N, dueling)
    err = np.abs(q[:B * A].double().numpy().reshape(B, A) - th.mean(-1))
    bound = ((3 * N + A + 4) if dueling else (N + 2)) * E24 * mag[:, None]
    print('q: max err / bound %.3f' % (err / bound).max())
    assert (err <= bound).all(), float((err / bound).max())
