"""Every forward and dgrad kernel of the Nature network, layer by layer, against float64
(tests/conv_ref.py: references, bound and its derivation), on all three builds, at B = 1, 2, 3.

Each layer is checked on the kernel's OWN stored input: x2 against conv2 of the x1 the kernel wrote, dz2
against the conv3 dgrad of the dz3 it wrote, and so on, so no ReLU flip and no rounding carries from one
layer into the next and every element of every tensor faces the per-element bound of ``conv_ref.check``
-- there is no tolerance beside it and no element is excluded. Weights are normal(0, 0.03), rounded to
the storage type in the 16-bit builds, written into the flat buffer and packed by ``executor.repack``: the
pack kernel's forward and dgrad fragments are under test with the kernels that read them. Pixels are
uint8 with 0 and 255 present and the outermost ring at 255. Every buffer a kernel writes lies between two
guard bands that must come back untouched and starts as NaN.

terms / extra_roundings per kernel (conv_ref's docstring has the rules):

  trunk_fwd_kernel   conv1 K = 256: one wave, 8 k-steps; scale and bias: 256 / 2. fp32 build: split3_bf16,
  (trunk.hip)        three exact bf16 MFMAs per k-step: 768 / 2 on S * SPLIT3_S.
                     conv2 K = 512, conv3 K = 576: two k-halves met in LDS (park / unpark: one more
                     addition, inside the count); scale is absent but counted with the bias: K / 2,
                     fp32 build K / 3 (product rounding).
  igemm C1 / F1      K = 256, one wave per tile, fp32 MFMAs on converted pixels in the fp32 build: 256 / 2 (3)
  igemm C2, C3       K = 512 / 576, KSPLIT 2 + LDS reduction: K / 2 (3)
  igemm DDGRAD       fc dgrad, K = 512, KSPLIT 4 + LDS reduction, mask select: 512 / 0 (1)
  igemm D3           DgradLoader, K = 9 x 64 = 576 (an invalid tap is an exact zero), KSPLIT 2: 576 / 0 (1)
  dgrad_s2_kernel    D2 by parity class: 4 taps x 64 = 256 terms in two halves met in LDS: 256 / 0 (1)
  igemm D2, generic  launch_igemm sends conv2's dgrad through the generic DgradLoader whenever the launch
                     carries a side duty; a zero range is one the binding accepts, so the test passes a
                     small one: 16 taps x 64 = 1024 k values, at most 256 of them real for any pixel;
                     checked under the SAME 256-term bound as the parity kernel.
  dgrad_chain_kernel the same three bodies in one launch: bit-equal to the separate launches.

The largest err / bound per kernel and build is printed (profiles/conv_layer_tests.txt keeps a copy). In
the 16-bit builds it sits near 1 by construction: the storage rounding (u |ref|) is most of the bound and
a round-to-nearest result lands anywhere up to half an ulp from its fp32 value. The fp32 build's figures
are the ones that show the accumulation term's slack.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

import conv_ref as cr

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
SENT = -4096.0                 # guard bands (exact in every type; no result is near it)
GUARD = 64
# variant -> (--dtype, act_t, kLossScale)
BUILDS = {'': ('bf16', torch.bfloat16, 1.0), 'f16': ('fp16', torch.float16, 1024.0),
          'f32': ('fp32', torch.float32, 1.0)}
SLOTS = [[3, 1, 1, 0], [5, 5, 2, 4], [0, 3, 2, 2]]
_ratios = {}


def note(kernel, variant, ratio):
    key = (kernel, BUILDS[variant][0])
    _ratios[key] = max(_ratios.get(key, 0.0), ratio)
    print('%-28s %-5s max err / bound %.3f (so far %.3f)' % (kernel, key[1], ratio, _ratios[key]))


class Buf:
    """n elements between two guard bands; the elements start as ``fill`` (NaN: never written)."""

    def __init__(self, n, dtype, fill=float('nan')):
        self.n = n
        self.all = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=DEV)
        self.t = self.all[GUARD:GUARD + n]
        self.t.fill_(fill)

    def data_ptr(self):
        return self.t.data_ptr()

    def get(self, what):
        """The elements (storage type, on the CPU) after checking both guard bands."""
        torch.cuda.synchronize()
        g = torch.cat([self.all[:GUARD], self.all[GUARD + self.n:]])
        assert bool((g == SENT).all()), '%s: a guard band was written' % what
        return self.t.cpu()


@functools.lru_cache(maxsize=None)
def make_net(kind, variant):
    """(net, executor, {tensor name: float64 CPU copy}) with the test's weights packed."""
    from dist_dqn_amd.config import preset
    from dist_dqn_amd.models.network import Network
    dtype, act_t, _ = BUILDS[variant]
    net = Network.create_network(preset(kind, 'Pong-v0', '--seed=0 --backend=hip --dtype=%s' % dtype), (84, 84, 4), 6,
                                 device=DEV)
    ex = net.executor
    assert ex.name == 'hip' and ex.act_dtype == act_t
    assert ex.ext.__name__.endswith({'': '_C', 'f16': '_C_f16', 'f32': '_C_f32'}[variant])
    flat = torch.randn(net.online.flat.numel(), generator=torch.Generator().manual_seed(11)) * 0.03
    flat = flat.to(act_t).float()                  # exact in the storage type: the pack kernel rounds nothing
    net.online.flat.copy_(flat)
    ex.repack(net.online.flat)
    torch.cuda.synchronize()
    lay = net.layout
    w = {n: flat[lay.offsets[n]:lay.offsets[n] + lay.numel(n)].double() for n in lay.names}
    return net, ex, w


def pixels(B, slots):
    """(kernel input, ring or None, float64 NHWC [B][84][84][4]): 0 and 255 present, the ring at 255."""
    g = torch.Generator().manual_seed(5 + B)
    if slots:
        ring = torch.randint(0, 256, (6, 84, 84), generator=g, dtype=torch.uint8)
        ring[:, 0], ring[:, -1], ring[:, :, 0], ring[:, :, -1] = 255, 255, 255, 255
        ring[:, 41, 43] = 0
        sl = torch.tensor(SLOTS[:B], dtype=torch.int32)
        x = ring[sl.long()].permute(0, 2, 3, 1).double()
        return sl.to(DEV), ring.to(DEV), x
    x8 = torch.randint(0, 256, (B, 84, 84, 4), generator=g, dtype=torch.uint8)
    x8[:, 0], x8[:, -1], x8[:, :, 0], x8[:, :, -1] = 255, 255, 255, 255
    x8[:, 41, 43] = 0
    return x8.to(DEV), None, x8.double()


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------ forward
def _forward(variant, B, slots, fused):
    net, ex, w = make_net('nature', variant)
    _, act_t, _ = BUILDS[variant]
    c1, c2, c3 = net.arch.convs
    inp, ring, x = pixels(B, slots)
    E = B - 1                                     # valid rows of the last instance (0: all of them)
    n1, n2, n3 = B * 400 * 32, B * 81 * 64, B * 49 * 64
    ninst = 3
    ws = {'x1': [Buf(n1, act_t) for _ in range(ninst)], 'x2': [Buf(n2, act_t) for _ in range(ninst)],
          'x3': [Buf(n3, act_t) for _ in range(ninst)]}
    use_m = fused and E > 0                       # (the layer-wise launches have one M for every instance)
    if use_m:
        ws['x3'][2].t[E * 49 * 64:] = SENT
    p, f = ex.packed(net.online.flat), net.online.flat
    ex.fused_trunk = fused
    try:
        ex._fwd_trunk([inp] * ninst, [p] * ninst, [f] * ninst, ws, B, ninst, frames=ring, fc=False,
                      M=(0, 0, E) if use_m else ())
        torch.cuda.synchronize()
    finally:
        ex.fused_trunk = True
    tag = '%s B%d %s' % ('trunk_fwd' if fused else 'igemm', B, 'slots' if slots else 'nhwc')
    x1 = ws['x1'][0].get(tag + ' x1').view(B, 20, 20, 32)
    x2 = ws['x2'][0].get(tag + ' x2').view(B, 9, 9, 64)
    x3 = ws['x3'][0].get(tag + ' x3').view(B, 7, 7, 64)
    fp32 = variant == 'f32'
    scale = f32(ex.input_scale)
    ref, S = cr.conv_fwd(x, w[c1.name + '/w'].view(256, 32), w[c1.name + '/b'], 8, 4, scale=scale)
    if fused and fp32:                            # split3_bf16: exact products, three terms each
        r = cr.check(x1, ref, S * cr.SPLIT3_S, 3 * 256, act_t, 2, tag + ' x1')
    else:
        r = cr.check(x1, ref, S, 256, act_t, 2 + fp32, tag + ' x1')
    kern = 'trunk_fwd_kernel' if fused else 'igemm %s' % ('F1' if slots else 'C1')
    note(kern + (' conv1' if fused else ''), variant, r)
    ref, S = cr.conv_fwd(x1.double(), w[c2.name + '/w'].view(512, 64), w[c2.name + '/b'], 4, 2)
    note(kern + ' conv2' if fused else 'igemm C2', variant, cr.check(x2, ref, S, 512, act_t, 2 + fp32, tag + ' x2'))
    ref, S = cr.conv_fwd(x2.double(), w[c3.name + '/w'].view(576, 64), w[c3.name + '/b'], 3, 1)
    note(kern + ' conv3' if fused else 'igemm C3', variant, cr.check(x3, ref, S, 576, act_t, 2 + fp32, tag + ' x3'))
    # the other instances: the same inputs and packs -> the same bits
    x3 = x3.reshape(-1)
    assert torch.equal(ws['x3'][1].get(tag + ' x3[1]'), x3), tag + ': instance 1 differs from instance 0'
    last = ws['x3'][2].get(tag + ' x3[2]')
    rows = E * 49 * 64 if use_m else n3
    assert torch.equal(last[:rows], x3[:rows]), tag + ': instance 2 differs from instance 0'
    assert bool((last[rows:] == SENT).all()), tag + ': rows >= M of the last instance were written'
    if fused:                                     # only the online instance keeps x1 / x2
        for k in ('x1', 'x2'):
            for i in (1, 2):
                assert bool(torch.isnan(ws[k][i].get(tag + ' ' + k)).all()), tag + ': %s of instance %d written' % (k, i)
    else:
        for k, own in (('x1', x1), ('x2', x2)):
            for i in (1, 2):
                assert torch.equal(ws[k][i].get(tag + ' ' + k), own.reshape(-1)), (tag, k, i)


@pytest.mark.parametrize('B', [1, 2, 3])
@pytest.mark.parametrize('slots', [False, True], ids=['nhwc', 'slots'])
@pytest.mark.parametrize('variant', ['', 'f16', 'f32'])
def test_fused_trunk_layers(variant, slots, B):
    """trunk_fwd_kernel (two row halves per sample, row groups packed across samples: B = 1 and odd B are
    its edges) from NHWC stacks and from frame-ring slot tables with repeated and out-of-order slots."""
    _forward(variant, B, slots, True)


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('slots', [False, True], ids=['nhwc', 'slots'])
@pytest.mark.parametrize('variant', ['', 'f16', 'f32'])
def test_layerwise_forward_layers(variant, slots, B):
    """fused_trunk = False: igemm kinds C1 / F1, C2, C3 (M = 400 B, 81 B, 49 B: partly filled last tiles)."""
    _forward(variant, B, slots, False)


# ------------------------------------------------------------------ backward
def _operands(variant, B):
    """Test-made x1, x2, x3 (>= 0, about half exactly zero) and dh (scaled by kLossScale), storage type."""
    _, act_t, loss = BUILDS[variant]
    g = torch.Generator().manual_seed(40 + B)
    act = lambda *s: torch.relu(torch.randn(*s, generator=g)).to(act_t)
    return dict(x1=act(B, 20, 20, 32), x2=act(B, 9, 9, 64), x3=act(B, 3136),
                dh=(torch.randn(B, 512, generator=g) * 0.1 * loss).to(act_t),
                parts=torch.rand(64, generator=g) + 0.5)


def _backward_ws(variant, B, ops):
    _, act_t, _ = BUILDS[variant]
    ws = {k: [ops[k].to(DEV).contiguous()] for k in ('x1', 'x2', 'x3')}
    ws['dh'] = ops['dh'].to(DEV).contiguous()
    ws['dz3'], ws['dz2'], ws['dz1'] = Buf(B * 3136, act_t), Buf(B * 81 * 64, act_t), Buf(B * 400 * 32, act_t)
    ws['loss_parts'] = ops['parts'].to(DEV)
    ws['loss'] = Buf(1, torch.float32)
    ws['zero'] = Buf(4 * 37, torch.float32, 7.0)
    return ws


def _state(ex, net, ws, B):
    po = ex.packed(net.online.flat)
    return SimpleNamespace(ws=ws, B=B, po=po, dev=DEV, zero=(ws['zero'].data_ptr(), ws['zero'].n),
                           pko=lambda key: po.data_ptr() + ex.esz * ex.poff[key])


def _side_duties(ws, ops, B, nparts, tag):
    assert bool((ws['zero'].get(tag + ' zero range') == 0).all()), tag + ': the zero range'
    want = float(ops['parts'][:nparts].double().sum()) / B
    got = float(ws['loss'].get(tag + ' loss')[0])
    assert abs(got - want) <= 8 * cr.EPS * abs(want), (tag, got, want)


@pytest.mark.parametrize('B', [1, 2, 3])
@pytest.mark.parametrize('variant', ['', 'f16', 'f32'])
def test_dgrad_layers(variant, B):
    """fc dgrad (DDGRAD with its side duties), conv3 dgrad (D3, the generic DgradLoader), conv2 dgrad (D2:
    dgrad_s2_kernel, whose last m-tile holds 4 of a class's 100 rows and whose taps with oy == OH or
    ox == OW must add nothing; and the generic loader, see the module docstring), each on the tensor the
    launch before it wrote; then dgrad_chain_kernel (two and three stages) bit-equal to them."""
    net, ex, w = make_net('nature', variant)
    _, act_t, _ = BUILDS[variant]
    fp32 = int(variant == 'f32')
    c1, c2, c3 = net.arch.convs
    ops = _operands(variant, B)
    ws = _backward_ws(variant, B, ops)
    st = _state(ex, net, ws, B)
    tag = 'dgrad B%d' % B
    # ---- fc dgrad, argument list as the executor builds it
    dh, pk, dz3p, x3p, dims, aux, aux_f = ex._fc_dgrad_args(ws, B, st.po, st.zero)
    ex.ext.qnet_igemm(6, [dh], [pk], [], [dz3p], [x3p], [1.0], dims, aux, aux_f)
    dz3 = ws['dz3'].get(tag + ' dz3')
    _side_duties(ws, ops, B, ex._loss_parts(B), tag)
    ref, S = cr.dense_dgrad(ops['dh'].double(), w['fcl/w'].view(3136, 512), ops['x3'].double())
    note('igemm DDGRAD (fc dgrad)', variant, cr.check(dz3.view(B, 3136), ref, S, 512, act_t, fp32, tag + ' dz3'))
    # (seven loss partials: the same dz3, the longer sum)
    ws['dz3'].t.fill_(float('nan'))
    ws['zero'].t.fill_(7.0)
    ex.ext.qnet_igemm(6, [dh], [pk], [], [dz3p], [x3p], [1.0], dims, aux[:3] + [7] + aux[4:], aux_f)
    assert torch.equal(ws['dz3'].get(tag + ' dz3 again'), dz3)
    _side_duties(ws, ops, B, 7, tag + ' 7 parts')
    # ---- conv3 dgrad of the kernel's dz3, conv2 dgrad of the kernel's dz2
    ex._conv_dgrad(st, 3)
    dz2 = ws['dz2'].get(tag + ' dz2')
    ref, S = cr.conv_dgrad(dz3.double().view(B, 7, 7, 64), w[c3.name + '/w'].view(576, 64), 3, 1, ops['x2'].double())
    note('igemm D3 (conv3 dgrad)', variant, cr.check(dz2.view(B, 9, 9, 64), ref, S, 576, act_t, fp32, tag + ' dz2'))
    ex._conv_dgrad(st, 2)
    dz1 = ws['dz1'].get(tag + ' dz1')
    ref, S = cr.conv_dgrad(dz2.double().view(B, 9, 9, 64), w[c2.name + '/w'].view(512, 64), 4, 2, ops['x1'].double())
    note('dgrad_s2_kernel (conv2 dgrad)', variant, cr.check(dz1.view(B, 20, 20, 32), ref, S, 256, act_t, fp32, tag + ' dz1'))
    # ---- conv2 dgrad through the generic loader (a launch with a side duty)
    ws['dz1'].t.fill_(float('nan'))
    ws['zero'].t.fill_(7.0)
    ex.ext.qnet_igemm(8, [ws['dz2'].data_ptr()], [st.pko('conv2/dgrad')], [], [ws['dz1'].data_ptr()],
                      [ws['x1'][0].data_ptr()], [1.0], ex._conv_dgrad_dims(B, 2), [st.zero[0], st.zero[1], 0, 0, 0], [1.0])
    gen = ws['dz1'].get(tag + ' dz1 generic')
    assert bool((ws['zero'].get(tag + ' zero range') == 0).all())
    note('igemm D2 (generic loader)', variant, cr.check(gen.view(B, 20, 20, 32), ref, S, 256, act_t, fp32, tag + ' dz1 generic'))
    # ---- the chained launch, through the executor
    assert ex.chain_dgrad == 0
    try:
        for stages in (1, 2):
            ex.chain_dgrad = stages
            assert ex.can_chain_dgrad(B)
            for k in ('dz3', 'dz2', 'dz1'):
                ws[k].t.fill_(float('nan'))
            ws['zero'].t.fill_(7.0)
            ws['loss'].t.fill_(float('nan'))
            ex._chain_ws(B, DEV).zero_()
            ex._dgrad_tail(st, SimpleNamespace(chain=True, dwg=True, noisy=False), None, None)
            t = '%s chain %d' % (tag, stages)
            assert torch.equal(ws['dz3'].get(t), dz3) and torch.equal(ws['dz2'].get(t), dz2), t
            assert torch.equal(ws['dz1'].get(t), dz1), t
            assert not ex.chain_error(B, DEV), t
            _side_duties(ws, ops, B, ex._loss_parts(B), t)
    finally:
        ex.chain_dgrad = 0
        ex._pending.wg = None
