"""tests/conv_ref.py can see the bugs it is for: at every layer geometry of the per-layer GPU tests and for
all three storage types, the checker accepts rounding noise and rejects a reference that is wrong by one
tap. No GPU.

The "kernel output" is the exact products (rounded to fp32 where the storage type is fp32) accumulated in
fp32 in a shuffled order, the fp32 epilogue (scale, bias, ReLU or the ReLU mask) and one rounding to the
storage type. The wrong variants go through the same arithmetic, so only their one defect separates them
from an accepted output. Each test prints the largest err / bound of the accepted output.
"""
import functools

import pytest
import torch

import conv_ref as cr

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
# forward geometries: input hw, cin, k, stride, cout, pads (top, bottom, left, right), u8 input, input scale
FWD = {
    'nature conv1': (84, 4, 8, 4, 32, (0, 0, 0, 0), True, 1.0 / 255.0),
    'nature conv2': (20, 32, 4, 2, 64, (0, 0, 0, 0), False, 1.0),
    'nature conv3': (9, 64, 3, 1, 64, (0, 0, 0, 0), False, 1.0),
    'cnn conv1': (84, 4, 8, 4, 32, (2, 2, 2, 2), True, 1.0),
    'cnn conv2': (11, 32, 4, 2, 64, (1, 2, 1, 2), False, 1.0),
    'cnn conv3': (3, 64, 3, 1, 64, (1, 1, 1, 1), False, 1.0),
}
# dgrad geometries: dz hw, cout, k, stride, input hw, cin, pads (top, left), ReLU mask in the launch
DGRAD = {
    'nature conv3 dgrad': (7, 64, 3, 1, 9, 64, (0, 0), True),
    'nature conv2 dgrad': (9, 64, 4, 2, 20, 32, (0, 0), True),
    'cnn conv3 dgrad': (3, 64, 3, 1, 3, 64, (1, 1), False),
    'cnn conv2 dgrad': (6, 64, 4, 2, 11, 32, (1, 1), False),
}
B = 2


def test_same_pads_are_the_layers():
    assert [cr.same_pads(84, 8, 4), cr.same_pads(11, 4, 2), cr.same_pads(3, 3, 1)] == [(2, 2), (1, 2), (1, 1)]
    assert [cr.same_pads(21, 2, 2), cr.same_pads(6, 2, 2), cr.same_pads(3, 2, 2)] == [(0, 1), (0, 0), (0, 1)]


# ------------------------------------------------------------------ inputs, exact in the storage type
def _gen(name, dt):
    return torch.Generator().manual_seed(sum(map(ord, name)) + DTYPES.index(dt))


def _acts(shape, dt, g, loss=1.0):
    """>= 0 with about half exactly zero (loss != 1: a signed gradient instead), as float64."""
    v = torch.randn(shape, generator=g)
    v = v * 0.1 * loss if loss != 1.0 else torch.relu(v)
    return v.to(dt).double()


def _pixels(b, g):
    x = torch.randint(0, 256, (b, 84, 84, 4), generator=g, dtype=torch.uint8)
    x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1] = 255, 255, 255, 255
    x[:, 40, 40] = 0
    return x.double()


def _weights(K, N, dt, g):
    return (torch.randn(K, N, generator=g) * 0.03).to(dt).double()


@functools.lru_cache(maxsize=None)
def _fwd_case(name, dt):
    hw, cin, k, s, n, pads, u8, scale = FWD[name]
    g = _gen(name, dt)
    x = _pixels(B, g) if u8 else _acts((B, hw, hw, cin), dt, g)
    w, b = _weights(k * k * cin, n, dt, g), (torch.randn(n, generator=g) * 0.1).double()
    ref, S = cr.conv_fwd(x, w, b, k, s, pads, scale)
    return dict(x=x, w=w, b=b, ref=ref, S=S, terms=k * k * cin, extra=2 + (dt == torch.float32))


@functools.lru_cache(maxsize=None)
def _dgrad_case(name, dt):
    ohw, co, k, s, ihw, cin, pads, mask = DGRAD[name]
    g = _gen(name, dt)
    dz = _acts((B, ohw, ohw, co), dt, g, loss=1024.0 if dt == torch.float16 else 2.0)
    x_in = _acts((B, ihw, ihw, cin), dt, g)
    w = _weights(k * k * cin, co, dt, g)
    ref, S = cr.conv_dgrad(dz, w, k, s, x_in, pads, mask)
    return dict(dz=dz, x_in=x_in, w=w, ref=ref, S=S, terms=k * k * co, extra=int(dt == torch.float32))


# ------------------------------------------------------------------ the simulated kernel
def _kernel(A, W, dt, g, scale=None, bias=None, keep=None):
    """fp32 accumulation of the products A[m][k] W[k][n] in a shuffled k order, then the fp32 epilogue
    (scale, bias, ReLU; or the mask ``keep``) and the rounding to ``dt``."""
    acc = torch.zeros(A.shape[0], W.shape[1], dtype=torch.float32)
    for kk in torch.randperm(A.shape[1], generator=g).tolist():
        acc = acc + (A[:, kk, None] * W[None, kk, :]).float()       # (float64 product, rounded once)
    if scale is not None:
        acc = torch.relu(acc * torch.tensor(scale, dtype=torch.float32) + bias.float())
    if keep is not None:
        acc = torch.where(keep, acc, torch.zeros_like(acc))
    return acc.to(dt).double()


def _run_fwd(name, dt, x=None, w=None, pads=None, edit=None):
    c = _fwd_case(name, dt)
    hw, cin, k, s, n, true_pads, _, scale = FWD[name]
    A, _ = cr.patches(c['x'] if x is None else x, k, s, true_pads if pads is None else pads)
    if edit is not None:
        A = edit(A.clone())
    out = _kernel(A, c['w'] if w is None else w, dt, _gen(name + 'k', dt), scale, c['b']).reshape(c['ref'].shape)
    return cr.check(out, c['ref'], c['S'], c['terms'], dt, c['extra'], name)


def _run_dgrad(name, dt, w=None, mask_src=None, edit=None):
    c = _dgrad_case(name, dt)
    ohw, co, k, s, ihw, cin, pads, mask = DGRAD[name]
    A = cr.dgrad_patches(c['dz'], k, s, (ihw, ihw), pads)
    Wd = cr.dgrad_weights(c['w'] if w is None else w, k, cin, co)
    keep = ((c['x_in'] if mask_src is None else mask_src) > 0).reshape(-1, cin) if mask else None
    out = _kernel(A, Wd, dt, _gen(name + 'k', dt), keep=keep)
    if edit is not None:
        out = edit(out, A, keep)
    return cr.check(out.reshape(c['ref'].shape), c['ref'], c['S'], c['terms'], dt, c['extra'], name)


# ------------------------------------------------------------------ rounding noise passes
@pytest.mark.parametrize('dt', DTYPES, ids=str)
@pytest.mark.parametrize('name', list(FWD))
def test_forward_rounding_noise_is_accepted(name, dt):
    r = _run_fwd(name, dt)
    print('%s %s: max err / bound %.3f' % (name, dt, r))
    assert r <= 1.0


@pytest.mark.parametrize('dt', DTYPES, ids=str)
@pytest.mark.parametrize('name', list(DGRAD))
def test_dgrad_rounding_noise_is_accepted(name, dt):
    r = _run_dgrad(name, dt)
    print('%s %s: max err / bound %.3f' % (name, dt, r))
    assert r <= 1.0


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_fc_dgrad_rounding_noise_is_accepted(dt):
    g = _gen('fc', dt)
    dh = _acts((3, 512), dt, g, loss=1024.0 if dt == torch.float16 else 2.0)
    x3, w = _acts((3, 3136), dt, g), _weights(3136, 512, dt, g)
    ref, S = cr.dense_dgrad(dh, w, x3)
    out = _kernel(dh, w.t(), dt, g, keep=x3 > 0)
    r = cr.check(out, ref, S, 512, dt, int(dt == torch.float32), 'fc dgrad')
    print('fc dgrad %s: max err / bound %.3f' % (dt, r))
    with pytest.raises(AssertionError):          # one hidden unit left out of one row
        dh2 = dh.clone()
        dh2[1, 77] = 0.0
        cr.check(_kernel(dh2, w.t(), dt, g, keep=x3 > 0), ref, S, 512, dt, int(dt == torch.float32), 'fc dgrad')


# ------------------------------------------------------------------ one-tap errors fail
@pytest.mark.parametrize('dt', DTYPES, ids=str)
@pytest.mark.parametrize('name,row,tap', [('nature conv1', 19, 6), ('cnn conv1', 0, 2 * 8 + 6), ('cnn conv3', 0, 4)])
def test_dropped_border_tap_is_rejected(name, row, tap, dt):
    """One (kh, kw) tap (every input channel) of ONE border output pixel of sample 0 contributes nothing:
    the top-right / top-left pixel of conv1 losing a tap on the image's first row (the ring of 255s),
    the corner pixel of the cnn's conv3 its centre tap."""
    cin = FWD[name][1]

    def drop(A):
        assert A[row, tap * cin:(tap + 1) * cin].abs().sum() > 0
        A[row, tap * cin:(tap + 1) * cin] = 0.0
        return A
    with pytest.raises(AssertionError):
        _run_fwd(name, dt, edit=drop)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
@pytest.mark.parametrize('name', ['nature conv3', 'cnn conv2'])
def test_swapped_kh_kw_is_rejected(name, dt):
    hw, cin, k, s, n = FWD[name][:5]
    w = _fwd_case(name, dt)['w'].reshape(k, k, cin, n).transpose(0, 1).reshape(k * k * cin, n)
    with pytest.raises(AssertionError):
        _run_fwd(name, dt, w=w)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
@pytest.mark.parametrize('name,pads', [('cnn conv2', (2, 1, 1, 2)), ('cnn conv1', (1, 3, 2, 2)), ('cnn conv3', (0, 2, 1, 1))])
def test_shifted_same_padding_is_rejected(name, pads, dt):
    """The SAME rows split one off the true (top, bottom): conv2's 1 / 2 taken as 2 / 1, conv1's 2 / 2 as
    1 / 3, conv3's 1 / 1 as 0 / 2."""
    assert pads != FWD[name][5] and sum(pads) == sum(FWD[name][5])
    with pytest.raises(AssertionError):
        _run_fwd(name, dt, pads=pads)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_parity_class_with_anothers_taps_is_rejected(dt):
    """Nature conv2 dgrad by parity: the input pixels of class (iy & 1, ix & 1) = (1, 0) computed with the
    weights of the taps of class (0, 0) (kh one less), every other class right."""
    name = 'nature conv2 dgrad'
    c = _dgrad_case(name, dt)
    w4 = c['w'].reshape(4, 4, 32, 64)
    wrong = cr.dgrad_weights(w4[[3, 0, 1, 2]].reshape(512, 64), 4, 32, 64)     # tap kh reads W[kh - 1]

    def one_class(out, A, keep):
        bad = _kernel(A, wrong, dt, _gen(name + 'w', dt), keep=keep).reshape(B, 20, 20, 32)
        out = out.reshape(B, 20, 20, 32).clone()
        out[:, 1::2, 0::2] = bad[:, 1::2, 0::2]
        return out.reshape(-1, 32)
    with pytest.raises(AssertionError):
        _run_dgrad(name, dt, edit=one_class)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
@pytest.mark.parametrize('name', ['nature conv3 dgrad', 'nature conv2 dgrad'])
def test_relu_mask_of_the_wrong_pixel_is_rejected(name, dt):
    x_in = _dgrad_case(name, dt)['x_in']
    with pytest.raises(AssertionError):
        _run_dgrad(name, dt, mask_src=torch.roll(x_in, 1, dims=2))      # the mask of the pixel one column left


# ------------------------------------------------------------------ max-pool
def _tied(hw, c, dt, g):
    """A pre-pool map from four values, zero among them: ties in every position pair of a window."""
    return (torch.randint(0, 4, (B, hw, hw, c), generator=g).double() * 0.5).to(dt).double()


def _pool_bwd_wrong(a, dp, last=False, wrap=False):
    """pool_bwd with a defect. last: the LAST maximum of a window gets the gradient. wrap: a cell right of
    the map's last column is read where a missing bounds check would read it, from the first column of
    the next row, and wins if it is the largest (its gradient then leaves the map)."""
    Bn, H, W, C = a.shape
    QH, QW = (H + 1) // 2, (W + 1) // 2
    ap = torch.full((Bn, 2 * QH, 2 * QW, C), float('-inf'), dtype=torch.float64)
    ap[:, :H, :W] = a
    if wrap and W % 2:
        ap[:, :H - 1, W] = a[:, 1:, 0]
    best = torch.full((Bn, QH, QW, C), float('-inf'), dtype=torch.float64)
    arg = torch.zeros((Bn, QH, QW, C), dtype=torch.int64)
    for i in range(4):
        v = ap[:, (i >> 1)::2, (i & 1)::2]
        better = (v >= best) if last else (v > best)
        better &= v > float('-inf')
        best, arg = torch.where(better, v, best), torch.where(better, torch.full_like(arg, i), arg)
    out = torch.zeros_like(ap)
    for i in range(4):
        out[:, (i >> 1)::2, (i & 1)::2] = torch.where((arg == i) & (best > 0), dp, torch.zeros_like(dp))
    return out[:, :H, :W].contiguous()


@pytest.mark.parametrize('hw,c', [(21, 32), (6, 64), (3, 64)])
def test_pool_forward_and_routing(hw, c):
    g = _gen('pool', torch.bfloat16)
    a = _tied(hw, c, torch.bfloat16, g)
    q = (hw + 1) // 2
    p = cr.pool_fwd(a)
    # against plain loops over the cells inside the map
    for py in range(q):
        for px in range(q):
            win = a[:, 2 * py:2 * py + 2, 2 * px:2 * px + 2].reshape(B, -1, c)
            assert torch.equal(p[:, py, px], win.max(1).values)
    assert bool(torch.isfinite(p).all())
    dp = torch.randn(B, q, q, c, generator=g).double()
    d = cr.pool_bwd(a, dp)
    # one cell per live window carries the whole gradient, it holds the maximum, no earlier cell does
    for py in range(q):
        for px in range(q):
            dw = d[:, 2 * py:2 * py + 2, 2 * px:2 * px + 2].reshape(B, -1, c)
            aw = a[:, 2 * py:2 * py + 2, 2 * px:2 * px + 2].reshape(B, -1, c)
            live = p[:, py, px] > 0
            assert torch.equal(dw.sum(1), torch.where(live, dp[:, py, px], torch.zeros_like(live, dtype=torch.float64)))
            assert torch.equal((dw != 0).sum(1) <= 1, torch.ones_like(live))
            first = (aw == p[:, py, px][:, None]).double().argmax(1)       # (argmax of 0 / 1: the first 1)
            sel = live & (dp[:, py, px] != 0)
            assert torch.equal((dw != 0).double().argmax(1)[sel], first[sel])


@pytest.mark.parametrize('dt', DTYPES, ids=str)
@pytest.mark.parametrize('defect', ['last', 'wrap'])
def test_pool_routing_defects_are_rejected(defect, dt):
    """cnn pool1 backward on a map with ties: the conv2 dgrad's fp32 result routed and rounded, as
    cnn_bwd_kernel forms dc1. The right routing passes; the last maximum, or a cell outside the map, fails."""
    name = 'cnn conv2 dgrad'
    c = _dgrad_case(name, dt)
    g = _gen('pool' + defect, dt)
    a1 = _tied(21, 32, dt, g)
    ref, S = cr.pool_bwd(a1, c['ref']), cr.pool_bwd(a1, c['S'])
    A = cr.dgrad_patches(c['dz'], 4, 2, (11, 11), (1, 1))
    acc = torch.zeros(A.shape[0], 32, dtype=torch.float32)
    Wd = cr.dgrad_weights(c['w'], 4, 32, 64)
    for kk in torch.randperm(A.shape[1], generator=g).tolist():
        acc = acc + (A[:, kk, None] * Wd[None, kk, :]).float()
    dp1 = acc.double().reshape(B, 11, 11, 32)
    right = cr.pool_bwd(a1, dp1).float().to(dt).double()
    r = cr.check(right, ref, S, c['terms'], dt, c['extra'], 'pool1 backward')
    print('pool1 backward %s: max err / bound %.3f' % (dt, r))
    wrong = _pool_bwd_wrong(a1, dp1, last=defect == 'last', wrap=defect == 'wrap').float().to(dt).double()
    assert not torch.equal(wrong, right)
    with pytest.raises(AssertionError):
        cr.check(wrong, ref, S, c['terms'], dt, c['extra'], 'pool1 backward')
