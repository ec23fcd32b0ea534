"""The reference ``cnn`` (csrc/kernels/cnn.hip: cnn_fwd_kernel, cnn_bwd_kernel) layer by layer against
float64 (tests/conv_ref.py), on all three builds, at B = 1 and 3; and the padded conv loaders of the
weight-gradient kernels, which only this network reaches.

Forward. a1, a2, a3 face ``conv_ref.check`` on the kernel's own previous tensor (the pixels, the p1 and p2
it stored), each with its SAME padding: 8x8 / 4 pad 2 | 2, 4x4 / 2 pad 1 | 2, 3x3 / 1 pad 1 | 1. p1, p2 and
the 256 features are the reference max-pool of the kernel's own a1, a2, a3 and must EQUAL it: the maximum
of stored values is one of them (21 -> 11 and 3 -> 2 end in a window of one row / one column).
terms / extra_roundings: conv1 256 / 2 (fp32 build: split3_bf16, 768 / 2 on S * SPLIT3_S); conv2 512 / 2
(one wave per tile, no K split); conv3 576 / 2 (two k-halves met in LDS); fp32 build + 1 (products).

Backward, ``qnet_cnn_bwd`` with the argument list ``HipCnnExecutor._backward`` builds, parts = 1, 2, 4, on
test-made a1, a2, a3 (about half zero; equal positive maxima planted in every position pair of a window,
the pattern changing with the window and the channel, so the bottom-row and right-column windows see
every pattern that fits them) and a test-made d(pool3 output). Each stage is recomputed from the kernel's
own stored upstream tensor (the second, tighter way the issue names):
  dc3   = pool3 backward of the given gradient: copies of stored values, must EQUAL the reference
          (first maximum in row-major order, nothing where that maximum is not > 0)
  dc2   = pool2 backward of the conv3 dgrad of the kernel's dc3: the dgrad's fp32 result is routed, then
          rounded, so the float64 dgrad and its S are routed by the same rule and checked: 576 / 0 (1)
  dc1   = pool1 backward of the conv2 dgrad of the kernel's dc2: 4 real taps x 64 = 256 / 0 (1); four
          parts split that sum in two K halves met in LDS (order, not count)
The bit-equality of parts = 2 with parts = 1 stays asserted in test_executor_gpu.py; here every part count
faces float64.

Padded weight gradients: ``qnet_wgrad`` with the dims ``_conv_member(..., pad=...)`` builds (84 -> 21 pad 2
from NHWC rows and from the frame ring, 11 -> 6 pad 1, 3 -> 3 pad 1) against the float64 patches of the
zero-padded input under test_wgrad_tiles_gpu.py's (M + 1) eps S bound, with its helpers.
"""
import pytest
import torch

import conv_ref as cr
from test_conv_layers_gpu import BUILDS, DEV, Buf, f32, make_net, note, pixels
from test_wgrad_tiles_gpu import L_C1, L_C2, L_C3, L_FRAMES, _dz, _layer, _reference

pytestmark = pytest.mark.gpu
PAD1, PAD2, PAD3 = (2, 2, 2, 2), (1, 2, 1, 2), (1, 1, 1, 1)
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('slots', [False, True], ids=['nhwc', 'slots'])
@pytest.mark.parametrize('variant', ['', 'f16', 'f32'])
def test_cnn_forward_layers(variant, slots, B):
    net, ex, w = make_net('atari', variant)
    assert type(ex).__name__ == 'HipCnnExecutor'
    _, act_t, _ = BUILDS[variant]
    c1, c2, c3 = net.arch.convs
    assert (c1.pads(), c2.pads(), c3.pads()) == (PAD1, PAD2, PAD3)
    inp, ring, x = pixels(B, slots)
    ninst = 3
    sizes = dict(a1=441 * 32, p1=121 * 32, a2=36 * 64, p2=9 * 64, a3=9 * 64)
    ws = {k: Buf(B * n, act_t) for k, n in sizes.items()}
    ws['x3'] = [Buf(B * 256, act_t) for _ in range(ninst)]
    p, f = ex.packed(net.online.flat), net.online.flat
    ex._fwd_trunk([inp] * ninst, [p] * ninst, [f] * ninst, ws, B, ninst, frames=ring, fc=False)
    tag = 'cnn_fwd B%d %s' % (B, 'slots' if slots else 'nhwc')
    a1 = ws['a1'].get(tag + ' a1').view(B, 21, 21, 32)
    p1 = ws['p1'].get(tag + ' p1').view(B, 11, 11, 32)
    a2 = ws['a2'].get(tag + ' a2').view(B, 6, 6, 64)
    p2 = ws['p2'].get(tag + ' p2').view(B, 3, 3, 64)
    a3 = ws['a3'].get(tag + ' a3').view(B, 3, 3, 64)
    x3 = ws['x3'][0].get(tag + ' x3').view(B, 2, 2, 64)
    fp32 = variant == 'f32'
    ref, S = cr.conv_fwd(x, w[c1.name + '/w'].view(256, 32), w[c1.name + '/b'], 8, 4, PAD1, f32(ex.input_scale))
    if fp32:
        r = cr.check(a1, ref, S * cr.SPLIT3_S, 3 * 256, act_t, 2, tag + ' a1')
    else:
        r = cr.check(a1, ref, S, 256, act_t, 2, tag + ' a1')
    note('cnn_fwd_kernel conv1', variant, r)
    assert torch.equal(p1.double(), cr.pool_fwd(a1.double())), tag + ': p1 is not the max-pool of a1'
    ref, S = cr.conv_fwd(p1.double(), w[c2.name + '/w'].view(512, 64), w[c2.name + '/b'], 4, 2, PAD2)
    note('cnn_fwd_kernel conv2', variant, cr.check(a2, ref, S, 512, act_t, 2 + fp32, tag + ' a2'))
    assert torch.equal(p2.double(), cr.pool_fwd(a2.double())), tag + ': p2 is not the max-pool of a2'
    ref, S = cr.conv_fwd(p2.double(), w[c3.name + '/w'].view(576, 64), w[c3.name + '/b'], 3, 1, PAD3)
    note('cnn_fwd_kernel conv3', variant, cr.check(a3, ref, S, 576, act_t, 2 + fp32, tag + ' a3'))
    assert torch.equal(x3.double(), cr.pool_fwd(a3.double())), tag + ': x3 is not the max-pool of a3'
    for i in (1, 2):
        assert torch.equal(ws['x3'][i].get(tag + ' x3[%d]' % i), x3.reshape(-1)), tag + ': instance %d differs' % i


# ------------------------------------------------------------------ backward
def _tied_acts(B, hw, c, act_t, g):
    """relu(randn) with equal positive maxima planted: window (py, px), channel ch takes pattern
    (7 py + 3 px + ch) % 16: the six position pairs of a window, and ten patterns that plant nothing
    (ties among zeros and single-cell windows come by themselves)."""
    q = (hw + 1) // 2
    ap = torch.zeros(B, 2 * q, 2 * q, c)
    ap[:, :hw, :hw] = torch.relu(torch.randn(B, hw, hw, c, generator=g))
    py, px, ch = torch.meshgrid(torch.arange(q), torch.arange(q), torch.arange(c), indexing='ij')
    pat = (7 * py + 3 * px + ch) % 16
    top = (4.0 + 0.25 * (ch % 4)).expand(B, q, q, c)           # above every other value, exact in every type
    for n, pair in enumerate(PAIRS):
        for i in pair:
            cell = ap[:, (i >> 1)::2, (i & 1)::2]
            cell[:] = torch.where((pat == n)[None].expand_as(cell), top, cell)
    return ap[:, :hw, :hw].contiguous().to(act_t)


@pytest.mark.parametrize('parts', [1, 2, 4])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('variant', ['', 'f16', 'f32'])
def test_cnn_backward_layers(variant, B, parts):
    net, ex, w = make_net('atari', variant)
    _, act_t, loss = BUILDS[variant]
    fp32 = int(variant == 'f32')
    c1, c2, c3 = net.arch.convs
    g = torch.Generator().manual_seed(70 + B)
    a1, a2, a3 = _tied_acts(B, 21, 32, act_t, g), _tied_acts(B, 6, 64, act_t, g), _tied_acts(B, 3, 64, act_t, g)
    for a in (a1, a2, a3):                        # the plan holds: zeros, and windows whose maximum is tied
        assert 0.3 < float((a == 0).float().mean()) < 0.6
    dp3 = (torch.randn(B, 256, generator=g) * 0.1 * loss).to(act_t)
    dev = [t.to(DEV).contiguous() for t in (dp3, a1, a2, a3)]
    dc1, dc2, dc3 = Buf(B * 441 * 32, act_t), Buf(B * 36 * 64, act_t), Buf(B * 9 * 64, act_t)
    po = ex.packed(net.online.flat)
    pko = lambda key: po.data_ptr() + ex.esz * ex.poff[key]
    ex.ext.qnet_cnn_bwd([dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                         pko('conv3/dgrad'), pko('conv2/dgrad'), dc1.data_ptr(), dc2.data_ptr(), dc3.data_ptr()], B,
                        prof=0, parts=parts)
    tag = 'cnn_bwd B%d parts%d' % (B, parts)
    k3 = dc3.get(tag + ' dc3').view(B, 3, 3, 64)
    k2 = dc2.get(tag + ' dc2').view(B, 6, 6, 64)
    k1 = dc1.get(tag + ' dc1').view(B, 21, 21, 32)
    a1, a2, a3 = a1.double(), a2.double(), a3.double()
    assert torch.equal(k3.double(), cr.pool_bwd(a3, dp3.double().view(B, 2, 2, 64))), tag + ': dc3 routing'
    d, S = cr.conv_dgrad(k3.double(), w[c3.name + '/w'].view(576, 64), 3, 1, torch.zeros(B, 3, 3, 64), (1, 1), mask=False)
    r = cr.check(k2, cr.pool_bwd(a2, d), cr.pool_bwd(a2, S), 576, act_t, fp32, tag + ' dc2')
    note('cnn_bwd_kernel conv3 dgrad+pool2', variant, r)
    d, S = cr.conv_dgrad(k2.double(), w[c2.name + '/w'].view(512, 64), 4, 2, torch.zeros(B, 11, 11, 32), (1, 1), mask=False)
    r = cr.check(k1, cr.pool_bwd(a1, d), cr.pool_bwd(a1, S), 256, act_t, fp32, tag + ' dc1')
    note('cnn_bwd_kernel conv2 dgrad+pool1', variant, r)


# ------------------------------------------------------------------ padded weight-gradient loaders
def _padded_case(layer, variant, frames=False):
    """B = 1, dims as ``HipCnnExecutor._backward`` hands them to ``_conv_member``."""
    _, act_t, _ = BUILDS[variant]
    ih, c, k, s, oh, n, pads = {1: (84, 4, 8, 4, 21, 32, PAD1), 2: (11, 32, 4, 2, 6, 64, PAD2),
                                3: (3, 64, 3, 1, 3, 64, PAD3)}[layer]
    g = torch.Generator().manual_seed(300 + layer)
    M, K = oh * oh, k * k * c
    dims = [M, n, K, 0, 0, ih, ih, oh, oh, pads[0], pads[2]]
    keep = []
    if layer == 1:
        inp, ring, x = pixels(1, frames)
        if frames:
            keep.append(ring)
            dims += [ring.data_ptr(), 84 * 84]
    else:
        xa = torch.relu(torch.randn(1, ih, ih, c, generator=g)).to(act_t)
        x, inp = xa.double(), xa.to(DEV)
    A, out_hw = cr.patches(x, k, s, pads)
    assert out_hw == (oh, oh)
    dz, dz64 = _dz(M, n, n, variant, g)
    kind = L_FRAMES if frames else {1: L_C1, 2: L_C2, 3: L_C3}[layer]
    return dict(kind=kind, inp=inp, dims=dims, dz=dz, ldz=n, M=M, K=K, N=n, keep=keep, **_reference(A, dz64))


@pytest.mark.parametrize('layer,frames', [(1, False), (1, True), (2, False), (3, False)])
@pytest.mark.parametrize('variant', ['', 'f16', 'f32'])
def test_padded_conv_wgrad(variant, layer, frames):
    """M = 441 (four 128-row chunks: atomics into zeros), 36 and 9 (one chunk, plain stores over NaN); the
    patches of the border output pixels reach into the SAME padding on every side."""
    scale = 0.5 if layer == 1 else 1.0
    c = _padded_case(layer, variant, frames)
    _layer(variant, c, 128, scale=scale).check(variant, 'padded conv%d%s' % (layer, ' frames' if frames else ''), scale)
