"""The per-layer and grouped weight-gradient launches (csrc/kernels/qnet.hip: wgrad_kernel,
wgrad_multi_kernel, wgrad_group_kernel) against a float64 reference, at the smallest shapes that
reach each tile edge, on all three builds.

The test drives ``ext.qnet_wgrad`` / ``ext.qnet_wgrad_group`` directly (argument layouts:
csrc/net_bindings.cpp ``wgrad`` / ``build_group``; dims as ``HipExecutor._conv_member`` builds them).
dW[k][n] = scale * sum_m A[m][k] dZ[m][n] / kLossScale and db[n] = sum_m dZ[m][n] / kLossScale, with
A the im2col patches of the Nature conv layers (u8 rows, the frame ring through a slot table with
repeated and out-of-order slots, NHWC activations) or dense rows.

Chunk sizes the cases are chosen against (a launch with more than one M-chunk accumulates with fp32
atomics into zeros; with one chunk it stores plainly, here over NaN):
  per-layer launch   conv 128 rows, dense 32 rows, the low-rank member 64 rows x mloop (plain stores)
  grouped launch     conv 256 rows (16-bit builds) / 128 rows (fp32 build), dense 32 rows;
                     deterministic partial members 128 rows x mloop per partial (16-bit builds only)

Sentinels: every output buffer ends in a guard band that must come back untouched; the gap between a
partial's K * N + N values and ``pstride`` likewise; ``db == nullptr`` leaves the weights correct.

Bound. Inputs are exact in the build's storage type and the reference is computed in float64 from the
same rounded values, so the only errors are: fp32 build, one rounding per product; every build, the
fp32 additions. A sum of M terms in any order (MFMA accumulation, per-thread bias partials, the
atomics across chunks into zero) passes each term through at most M - 1 inexact additions (adding to
an exact zero is exact), each with relative error at most eps = 2^-23 whatever the rounding mode of
the MFMA's internal adder, so to first order |err| <= (M - 1) eps S with S = sum_m |a dz|; one more
eps for the fp32 build's product rounding, and (1 + eps)^M - 1 <= 1.001 M eps at these M. The bound is
(M + 1) eps S: c = 1. ``scale`` is a power of two and the fp16 build's kInvLossScale is 2^-10: both
exact, applied to reference and bound alike. The largest err / bound per build is printed.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
EPS = 2.0 ** -23
SENT = -4096.0                 # guard bands (exact in every type; no result is near it)
GUARD = 64
# variant -> (act_t, kLossScale)
BUILDS = {'': (torch.bfloat16, 1.0), 'f16': (torch.float16, 1024.0), 'f32': (torch.float32, 1.0)}
L_C1, L_C2, L_C3, L_DENSE, L_FRAMES, L_HEAD, L_LR = 1, 2, 3, 4, 9, 11, 12
# Nature geometry: layer -> (IH, IW, CIN, KH, S, OH, OW, COUT)
GEO = {1: (84, 84, 4, 8, 4, 20, 20, 32), 2: (20, 20, 32, 4, 2, 9, 9, 64), 3: (9, 9, 64, 3, 1, 7, 7, 64)}
SLOTS = [[3, 1, 1, 0], [5, 5, 2, 4], [0, 3, 2, 2]]
_ratios = {}


def _ext(variant):
    from dist_dqn_amd.ops import _ext as loader
    return loader.load(required=True, variant=variant)


# ------------------------------------------------------------------ inputs and float64 references
def _reference(A, dz):
    """A [M][K], dz [M][N] float64 -> dW, its absolute sum, db, its absolute sum."""
    return dict(w=A.t() @ dz, aw=A.abs().t() @ dz.abs(), b=dz.sum(0), ab=dz.abs().sum(0))


def _dz(M, N, ldz, variant, g, pad=0.0):
    """dZ rows [M][ldz] in the build's type (scaled by kLossScale as the head leaves them), columns
    >= N holding ``pad``; and the float64 values of the first N columns without the scale."""
    act_t, loss = BUILDS[variant]
    z = torch.full((M, ldz), pad)
    z[:, :N] = torch.randn(M, N, generator=g) * 0.1 * loss
    z = z.to(act_t)
    return z.to(DEV).contiguous(), z[:, :N].double() / loss


@functools.lru_cache(maxsize=None)
def _conv_case(layer, B, variant, frames=False):
    IH, IW, C, KH, S, OH, OW, N = GEO[layer]
    act_t, _ = BUILDS[variant]
    g = torch.Generator().manual_seed(100 * layer + B)
    M, K = B * OH * OW, KH * KH * C
    keep = []
    dims = [M, N, K, 0, 0, IH, IW, OH, OW, 0, 0]
    if layer == 1 and frames:
        ring = torch.randint(0, 256, (6, IH * IW), generator=g, dtype=torch.uint8)
        slots = torch.tensor(SLOTS[:B], dtype=torch.int32)
        x = ring[slots.long()].view(B, 4, IH, IW).permute(0, 2, 3, 1).double()
        ring_d, inp = ring.to(DEV), slots.to(DEV)
        keep.append(ring_d)
        dims += [ring_d.data_ptr(), IH * IW]
    elif layer == 1:
        x8 = torch.randint(0, 256, (B, IH, IW, C), generator=g, dtype=torch.uint8)
        x, inp = x8.double(), x8.to(DEV)
    else:
        xa = torch.relu(torch.randn(B, IH, IW, C, generator=g)).to(act_t)
        x, inp = xa.double(), xa.to(DEV)
    A = x.unfold(1, KH, S).unfold(2, KH, S).permute(0, 1, 2, 4, 5, 3).reshape(M, K)     # k = (kh, kw, ci)
    dz, dz64 = _dz(M, N, N, variant, g)
    kind = L_FRAMES if frames else layer
    return dict(kind=kind, inp=inp, dims=dims, dz=dz, ldz=N, M=M, K=K, N=N, keep=keep, **_reference(A, dz64))


@functools.lru_cache(maxsize=None)
def _dense_case(kind, M, K, N, ldz, variant, pad=0.0):
    act_t, _ = BUILDS[variant]
    g = torch.Generator().manual_seed(7 * M + K + N + kind)
    xa = torch.relu(torch.randn(M, K, generator=g)).to(act_t)
    dz, dz64 = _dz(M, N, ldz, variant, g, pad)
    return dict(kind=kind, inp=xa.to(DEV), dims=[M, N, K, 0, 0, 0, 0, 0, 0, 0, 0], dz=dz, ldz=ldz, M=M, K=K, N=N,
                keep=[], **_reference(xa.double(), dz64))


# ------------------------------------------------------------------ outputs with sentinels
class _Out:
    """n floats (NaN under plain stores, zeros under accumulation) followed by a guard band."""

    def __init__(self, n, plain):
        self.n = n
        self.buf = torch.full((n + GUARD,), SENT, device=DEV)
        self.buf[:n] = float('nan') if plain else 0.0

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def get(self, what):
        assert bool((self.buf[self.n:] == SENT).all()), '%s: the guard band was written' % what
        return self.buf[:self.n].double().cpu()


class _Grads:
    """dw / db (/ dw2 / db2) of one member, split at nsplit."""

    def __init__(self, c, plain, nsplit=None, with_db=True):
        self.c, self.nsplit = c, c['N'] if nsplit is None else nsplit
        n1, n2 = self.nsplit, c['N'] - self.nsplit
        self.dw, self.db = _Out(c['K'] * n1, plain), _Out(n1, plain) if with_db else None
        self.dw2 = _Out(c['K'] * n2, plain) if n2 else None
        self.db2 = _Out(n2, plain) if n2 and with_db else None

    def ptrs(self):
        p = lambda o: o.ptr if o is not None else 0
        return [self.dw.ptr, p(self.db), p(self.dw2), p(self.db2), self.nsplit, self.c['N']]

    def check(self, variant, tag, scale=1.0, db_zero=False):
        c, K = self.c, self.c['K']
        w = self.dw.get(tag + ' dw').view(K, self.nsplit)
        if self.dw2 is not None:
            w = torch.cat([w, self.dw2.get(tag + ' dw2').view(K, -1)], 1)
        _compare(variant, tag + ' dW', w, c['w'] * scale, c['aw'] * scale, c['M'])
        if self.db is not None:
            b = self.db.get(tag + ' db')
            if self.db2 is not None:
                b = torch.cat([b, self.db2.get(tag + ' db2')])
            if db_zero:
                assert bool((b == 0).all()), tag + ': db_zero'
            else:
                _compare(variant, tag + ' db', b, c['b'], c['ab'], c['M'])
        return w


def _compare(variant, tag, got, ref, absum, M):
    assert bool(torch.isfinite(got).all()), '%s: an element was left unwritten (or is not finite)' % tag
    bound = (M + 1) * EPS * absum
    err = (got - ref).abs()
    ratio = float(torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())
    _ratios[variant] = max(_ratios.get(variant, 0.0), ratio)
    print('%s %r: max err / bound %.3f (build so far %.3f)' % (tag, variant, ratio, _ratios[variant]))
    bad = err > bound
    assert not bool(bad.any()), (tag, int(bad.sum()), [(idx.tolist(), float(got[tuple(idx)]), float(ref[tuple(idx)]))
                                                       for idx in bad.nonzero()[:5]])


# ------------------------------------------------------------------ per-layer launch
def _layer(variant, c, chunk, nsplit=None, with_db=True, scale=1.0, mloop=1, db_zero=False, plain=None):
    plain = (c['M'] + chunk - 1) // chunk == 1 if plain is None else plain
    gr = _Grads(c, plain, nsplit, with_db)
    # (MC / KB / NB and atomic are spelled as the executor spells them; the launcher picks its own)
    _ext(variant).qnet_wgrad(c['kind'], c['inp'].data_ptr(), c['dims'], c['dz'].data_ptr(), c['ldz'], *gr.ptrs(),
                             32, 64, 64, scale, True, mloop=mloop, db_zero=db_zero)
    torch.cuda.synchronize()
    return gr


@pytest.mark.parametrize('layer,frames', [(1, False), (1, True), (2, False), (3, False)])
@pytest.mark.parametrize('B', [1, 3])
def test_conv_layer_wgrad(layer, frames, B):
    """M = 400 / 1200 (conv1: u8 rows and the frame ring), 81 / 243 (conv2), 49 / 147 (conv3) in 128-row
    chunks: one chunk, several with a partly filled last one; conv1 carries a scale (the input scale)."""
    scale = 0.5 if layer == 1 else 1.0
    _layer('', _conv_case(layer, B, '', frames), 128, scale=scale).check('', 'conv%d B%d' % (layer, B), scale)


@pytest.mark.parametrize('M', [1, 31, 32, 33])
@pytest.mark.parametrize('nsplit', [128, 256])
def test_dense_layer_wgrad(M, nsplit):
    """L_DENSE_FWD_RELU, 32-row chunks around the chunk edge, with and without the dueling split."""
    _layer('', _dense_case(L_DENSE, M, 128, 256, 256, ''), 32, nsplit=nsplit).check('', 'dense M%d' % M)


@pytest.mark.parametrize('N,M', [(1, 7), (6, 7), (19, 33), (32, 7)])
def test_head_layer_wgrad(N, M):
    """L_HEAD_WGRAD: N columns of a 64-wide dZ; the columns past N hold 77 and must not show."""
    _layer('', _dense_case(L_HEAD, M, 128, N, 64, '', 77.0), 32).check('', 'head N%d' % N)


@pytest.mark.parametrize('mloop', [1, 3, 5])
def test_lowrank_member(mloop):
    """L_DENSE_WGRAD_LR: mloop 64-row chunks in one block per tile (5 crosses a 4-chunk load batch), M
    no multiple of 64, K no multiple of the 32-row K-range, N of the 64-column N-range; plain stores;
    db_zero stores zeros into the bias and leaves dW bit-equal."""
    c = _dense_case(L_LR, 64 * mloop - 23, 104, 72, 72, '')
    w = _layer('', c, 64, mloop=mloop, plain=True).check('', 'lowrank mloop%d' % mloop)
    w0 = _layer('', c, 64, mloop=mloop, plain=True, db_zero=True).check('', 'lowrank db_zero', db_zero=True)
    assert torch.equal(w, w0)


def test_layer_wgrad_without_bias():
    """db == nullptr: the weights of an accumulating conv launch and a plain dense launch stay correct."""
    _layer('', _conv_case(2, 3, ''), 128, with_db=False).check('', 'conv2 no db')
    _layer('', _dense_case(L_DENSE, 31, 128, 256, 256, ''), 32, nsplit=128, with_db=False).check('', 'dense no db')


# ------------------------------------------------------------------ grouped launch
def _nature_group(variant, B, frames):
    return [_conv_case(1, B, variant, frames), _conv_case(3, B, variant), _conv_case(2, B, variant),
            _dense_case(L_DENSE, B, 128, 256, 256, variant), _dense_case(L_HEAD, B, 128, 6, 64, variant, 77.0)]


def _group(variant, cases, with_db=True):
    """One grouped launch over ``cases`` (conv1 first: scale 0.5); the fc member with the dueling split."""
    conv_chunk = 128 if variant == 'f32' else 256
    grads, members, dims = [], [], []
    for c in cases:
        chunk = conv_chunk if c['kind'] in (L_C1, L_C2, L_C3, L_FRAMES) else 32
        gr = _Grads(c, (c['M'] + chunk - 1) // chunk == 1, 128 if c['kind'] == L_DENSE else None, with_db)
        grads.append(gr)
        members.append([c['kind'], c['inp'].data_ptr(), c['dz'].data_ptr(), c['ldz'], *gr.ptrs()])
        dims.append(c['dims'])
    _ext(variant).qnet_wgrad_group(members, dims, [0.5] + [1.0] * (len(cases) - 1))
    torch.cuda.synchronize()
    return grads


def _check_group(variant, B, frames, with_db=True):
    for i, gr in enumerate(_group(variant, _nature_group(variant, B, frames), with_db)):
        gr.check(variant, 'group B%d member %d' % (B, i), 0.5 if i == 0 else 1.0)


@pytest.mark.parametrize('B,frames', [(1, False), (3, True)])
def test_nature_group(B, frames):
    """conv1, conv3, conv2, fc, head in one call: 256-row conv chunks (128 in the fp32 build) with one
    chunk (plain stores) and several (atomics), beside the 32-row dense members."""
    _check_group('', B, frames)


def test_nature_group_without_bias():
    _check_group('', 3, False, with_db=False)


def _partials(variant, B, mloop):
    """The conv members as deterministic partial members: (case, partial buffer, groups, pstride)."""
    ext, out, members, dims = _ext(variant), [], [], []
    for c in (_conv_case(1, B, variant, True), _conv_case(3, B, variant), _conv_case(2, B, variant)):
        K, N = c['K'], c['N']
        gx = ((c['M'] + 127) // 128 + mloop - 1) // mloop
        pstride = K * N + N + 24
        part = _Out(gx * pstride, True)
        dw, db = _Out(K * N, True), _Out(N, True)        # (a partial member's own dw / db are not written)
        members.append([c['kind'], c['inp'].data_ptr(), c['dz'].data_ptr(), c['ldz'], dw.ptr, db.ptr, 0, 0, N, N,
                        part.ptr, pstride, mloop])
        dims.append(c['dims'])
        out.append((c, part, gx, pstride, dw, db))
    ext.qnet_wgrad_group(members, dims, [0.5, 1.0, 1.0])
    torch.cuda.synchronize()
    return out


def _check_partials(variant, B, mloop):
    first = _partials(variant, B, mloop)
    again = _partials(variant, B, mloop)
    for i, ((c, part, gx, pstride, dw, db), (_, part2, _, _, _, _)) in enumerate(zip(first, again)):
        tag = 'partials B%d mloop%d member %d' % (B, mloop, i)
        K, N, scale = c['K'], c['N'], 0.5 if i == 0 else 1.0
        p = part.get(tag).view(gx, pstride)
        assert bool(torch.isnan(p[:, K * N + N:]).all()), tag + ': the gap after a partial was written'
        assert bool(torch.isnan(dw.get(tag)).all()) and bool(torch.isnan(db.get(tag)).all()), tag + ': own dw / db'
        assert torch.equal(part.buf.view(torch.int32), part2.buf.view(torch.int32)), tag + ': two launches differ'
        _compare(variant, tag + ' dW', p[:, :K * N].sum(0).view(K, N), c['w'] * scale, c['aw'] * scale, c['M'])
        _compare(variant, tag + ' db', p[:, K * N:K * N + N].sum(0), c['b'], c['ab'], c['M'])


@pytest.mark.parametrize('B,mloop', [(1, 1), (3, 1), (3, 2), (3, 3)])
def test_partial_members(B, mloop):
    """Deterministic partial members: chunk groups of mloop 128-row chunks, one plain-stored partial each
    (pstride above K * N + N), summed here; two launches agree bit for bit."""
    _check_partials('', B, mloop)


# ------------------------------------------------------------------ the other builds, every body
@pytest.mark.parametrize('variant', ['f16', 'f32'])
def test_other_builds(variant):
    _layer(variant, _conv_case(1, 3, variant, True), 128, scale=0.5).check(variant, 'conv1 frames', 0.5)
    _layer(variant, _conv_case(2, 3, variant), 128).check(variant, 'conv2')
    _layer(variant, _conv_case(3, 1, variant), 128).check(variant, 'conv3')
    _layer(variant, _dense_case(L_DENSE, 33, 128, 256, 256, variant), 32, nsplit=128).check(variant, 'dense')
    _layer(variant, _dense_case(L_HEAD, 7, 128, 6, 64, variant, 77.0), 32).check(variant, 'head')
    _layer(variant, _dense_case(L_LR, 297, 104, 72, 72, variant), 64, mloop=5, plain=True).check(variant, 'lowrank')
    _check_group(variant, 3, True)
    _check_group(variant, 1, False)
    if variant == 'f32':
        # (the fp32 build has no deterministic partial members: refused before any launch)
        with pytest.raises(RuntimeError, match='partial members'):
            _partials(variant, 3, 2)
        torch.cuda.synchronize()
    else:
        _check_partials(variant, 3, 2)
