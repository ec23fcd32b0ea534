"""The two clip kernels (csrc/kernels/grad_clip.hip) in all three builds, against float64 on the fp32
inputs.

``grad_clip(grad, C, grad_scale, stats, partials, counter)`` writes ``stats = [norm, scale]`` with
``norm = grad_scale * ||grad||_2`` and ``scale = C / max(norm, C)`` (0 when the norm is not finite) and
multiplies ``grad`` by ``scale`` in place. The flat gradient carries no loss scale in any build (every
weight-gradient kernel of the fp16 build divides it out when it stores, csrc/include/dqn_act.h), so the
effective gradient is ``grad * grad_scale`` in the fp16 build as in the others.

Error bound on ``norm``, from the kernel's summation shape and u = 2^-24 (fp32 unit roundoff). With G =
``grad_clip_blocks(n)`` blocks of 256 threads, a thread sums its ceil(n4 / 256 G) float4s (n4 aligned
float4s in the slice), four squares each, plus at most one head / tail scalar: L additions. A wave
adds 4 DPP levels + 2 readlane levels, a block 2 more; the last block's threads each add ceil(G / 256)
partials and reduce the same way (6 + 2). With the squaring itself every term passes through at most
D = 1 + L + 8 + ceil(G / 256) + 8 roundings, and all terms are >= 0, so the computed sum of squares is
within gamma_D = D u / (1 - D u) of the exact one, relatively; the square root halves that and adds
at most 2 u, the product with grad_scale u. Below the normal range an operation may also lose up to
eta = 2^-126 absolutely (flush to zero; gradual underflow loses less): at most
N = 2 n + 257 G + 256 operations feed the result, and |sqrt(S + d) - sqrt(S)| <= sqrt(|d|). So

    |norm - norm64| <= (gamma_D / 2 + 3 u) norm64 + grad_scale sqrt(N eta).

No case is excluded. The largest error / bound ratio per build is printed.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
U = 2.0 ** -24
ETA = 2.0 ** -126
BUILDS = ['', 'f16', 'f32']
DATA = ['normal', 'zeros', 'huge', 'underflow']


def _ext(variant):
    from dist_dqn_amd.ops import _ext
    return _ext.load(required=True, variant=variant)


def _nature_total():
    from dist_dqn_amd.config import preset
    from dist_dqn_amd.models.arch import arch_from_config
    from dist_dqn_amd.models.params import FlatLayout
    return FlatLayout(arch_from_config(preset('nature', 'Pong-v0'), (84, 84, 4), 6)).total


def _sizes():
    return [1, 3, 4, 5, 63, 64, 65, 255, 1024, 4099, (1 << 20) + 4, _nature_total()]


def _bound(ext, n, off, norm64, grad_scale):
    G = int(ext.grad_clip_blocks(n))
    head = min(n, (4 - off % 4) % 4)
    n4 = (n - head) // 4
    L = 4 * -(-n4 // (256 * G)) + 1
    D = 1 + L + 8 + -(-G // 256) + 8
    gamma = D * U / (1.0 - D * U)
    N = 2 * n + 257 * G + 256
    return (gamma / 2 + 3 * U) * norm64 + grad_scale * math.sqrt(N * ETA)


def _data(kind, n, gen):
    if kind == 'normal':
        return torch.randn(n, device=DEV, generator=gen)
    if kind == 'zeros':
        return torch.zeros(n, device=DEV)
    if kind == 'huge':                         # one 3e18 (its square 9e36 is finite) among 1e-3-sized values
        x = torch.randn(n, device=DEV, generator=gen) * 1e-3
        x[n // 2] = 3e18
        return x
    assert kind == 'underflow'                 # squares below the fp32 normal range (some below 2^-149)
    return torch.randn(n, device=DEV, generator=gen) * 1e-21


class _Bufs:
    def __init__(self, ext, nmax):
        self.ext = ext
        self.stats = torch.zeros(2, device=DEV)
        self.partials = torch.zeros(int(ext.grad_clip_blocks(nmax)), device=DEV)
        self.counter = torch.zeros(1, dtype=torch.int32, device=DEV)

    def clip(self, g, C, gs=1.0):
        self.ext.grad_clip(g, float(C), float(gs), self.stats, self.partials, self.counter)
        return self.stats


def _sliced(x, off):
    """x's values in a slice that starts ``off`` elements past a 16-byte boundary, with 4 + off guard
    elements before it and 8 after."""
    n = x.numel()
    big = torch.full((n + 12 + off,), 7.25, device=DEV)
    assert big.data_ptr() % 16 == 0
    lo = 4 + off
    big[lo:lo + n] = x
    return big, big[lo:lo + n], lo


@pytest.mark.parametrize('variant', BUILDS)
def test_norm_scale_and_scaled_values_at_every_size_alignment_and_data_set(variant):
    ext = _ext(variant)
    sizes = _sizes()
    bufs = _Bufs(ext, max(sizes))
    gen = torch.Generator(device=DEV).manual_seed(11)
    worst = (0.0, None)
    for n in sizes:
        assert 1 <= int(ext.grad_clip_blocks(n)) <= 512
        for off in range(4):
            for kind in DATA:
                x = _data(kind, n, gen)
                norm64 = float(x.double().pow(2).sum().sqrt())
                for rel in (0.5, 10.0):                      # clipping active / inactive
                    C = rel * norm64 if norm64 > 1e-30 else 1.0
                    big, g, lo = _sliced(x, off)
                    ref = big.clone()
                    st = bufs.clip(g, C).cpu()
                    norm, scale = float(st[0]), float(st[1])
                    bound = _bound(ext, n, off, norm64, 1.0)
                    err = abs(norm - norm64)
                    case = (variant, n, off, kind, rel)
                    if err / bound > worst[0]:
                        worst = (err / bound, case)
                    assert err <= bound, (case, norm, norm64, err, bound)
                    assert int(bufs.counter) == 0, case
                    # guards untouched
                    assert torch.equal(big[:lo], ref[:lo]) and torch.equal(big[lo + n:], ref[lo + n:]), case
                    # scale is the fp32 formula on the reported norm (C rounded to fp32, one division)
                    c32 = float(torch.tensor(C, dtype=torch.float32))
                    mine = c32 / max(norm, c32)
                    assert abs(scale - mine) <= 2 * U * mine and (scale == 1.0) == (norm <= c32), (case, scale, mine)
                    if scale == 1.0:
                        assert torch.equal(big, ref), case           # the same bits
                    else:
                        # every element is fp32(x * scale), exactly
                        assert torch.equal(g.cpu(), torch.from_numpy(x.cpu().numpy() * st[1].numpy())), case
                    # and it is float64's, wherever the norm's bound leaves no doubt which side of C it is
                    if norm64 + bound <= C:
                        assert scale == 1.0, case
                    elif norm64 - bound > C:
                        want = C / norm64
                        assert abs(scale - want) <= want * (bound / norm64 + 3 * U), (case, scale, want)
                    else:
                        assert kind == 'underflow', case              # (only there is the bound that wide)
    print('grad_clip %s: largest |norm - norm64| / bound = %.4f at %s' % (variant or 'bf16', worst[0], worst[1]))


@pytest.mark.parametrize('variant', BUILDS)
def test_grad_scale_is_part_of_the_norm(variant):
    """norm = ||grad * grad_scale||: the data-parallel average (1/8 here) as the optimizer applies it. The
    fp16 build's flat gradient carries no loss scale (dqn_act.h), so its expectation is the same."""
    ext = _ext(variant)
    n = 4099
    bufs = _Bufs(ext, n)
    x = torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    norm64 = float((x.double() / 8).pow(2).sum().sqrt())
    for rel in (0.5, 10.0):
        g = x.clone()
        st = bufs.clip(g, rel * norm64, 0.125).cpu()
        bound = _bound(ext, n, 0, norm64, 0.125)
        assert abs(float(st[0]) - norm64) <= bound
        if rel > 1:
            assert float(st[1]) == 1.0 and torch.equal(g, x)
        else:
            assert abs(float(st[1]) - 0.5) <= 0.5 * (bound / norm64 + 3 * U)
            assert torch.equal(g, x * bufs.stats[1]), 'the buffer is scaled by scale alone (not by grad_scale)'


@pytest.mark.parametrize('variant', BUILDS)
def test_same_bits_on_every_call_and_every_graph_replay(variant):
    ext = _ext(variant)
    n = _nature_total()
    bufs = _Bufs(ext, n)
    x = torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    g = x.clone()
    C = 0.5 * float(x.double().norm())
    seen = set()
    for _ in range(20):
        g.copy_(x)
        st = bufs.clip(g, C)
        seen.add(tuple(st.view(torch.int32).tolist()))
    assert len(seen) == 1, seen
    first = g.clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(graph, stream=s):
        g.copy_(x)
        bufs.clip(g, C)
    torch.cuda.current_stream(DEV).wait_stream(s)
    for _ in range(20):
        bufs.stats.zero_()
        graph.replay()
        seen.add(tuple(bufs.stats.view(torch.int32).tolist()))
        assert int(bufs.counter) == 0, 'the arrival counter resets itself'
    assert len(seen) == 1, seen
    assert torch.equal(g, first)


@pytest.mark.parametrize('variant', BUILDS)
@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_non_finite_input_gives_scale_zero_and_a_zeroed_buffer(variant, bad):
    ext = _ext(variant)
    for n, off in ((5, 1), (4099, 3), ((1 << 20) + 4, 2)):
        bufs = _Bufs(ext, n)
        x = torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
        x[n - 2] = bad
        big, g, lo = _sliced(x, off)
        st = bufs.clip(g, 10.0).cpu()
        assert not math.isfinite(float(st[0])), 'the norm is reported as computed'
        assert float(st[1]) == 0.0
        assert torch.equal(g, torch.zeros_like(g))
        assert bool((big[:lo] == 7.25).all()) and bool((big[lo + n:] == 7.25).all())
        assert int(bufs.counter) == 0


@pytest.mark.parametrize('variant', BUILDS)
def test_binding_refuses_bad_arguments(variant):
    ext = _ext(variant)
    bufs = _Bufs(ext, 1 << 16)
    g = torch.ones(1 << 16, device=DEV)
    ok = (bufs.stats, bufs.partials, bufs.counter)
    with pytest.raises(RuntimeError, match='dtype'):
        ext.grad_clip(g.half(), 1.0, 1.0, *ok)
    with pytest.raises(RuntimeError, match='dtype'):
        ext.grad_clip(g, 1.0, 1.0, bufs.stats.double(), bufs.partials, bufs.counter)
    for c in (0.0, -1.0, float('nan')):
        with pytest.raises(RuntimeError, match='max_norm'):
            ext.grad_clip(g, c, 1.0, *ok)
    with pytest.raises(RuntimeError, match='stats'):
        ext.grad_clip(g, 1.0, 1.0, bufs.stats[:1], bufs.partials, bufs.counter)
    with pytest.raises(RuntimeError, match='partials'):
        ext.grad_clip(g, 1.0, 1.0, bufs.stats, bufs.partials[:int(ext.grad_clip_blocks(1 << 16)) - 1], bufs.counter)
    with pytest.raises(RuntimeError, match='contiguous'):
        ext.grad_clip(g[::2], 1.0, 1.0, *ok)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ext.grad_clip(g.cpu(), 1.0, 1.0, *ok)
    with pytest.raises(RuntimeError, match='empty'):
        ext.grad_clip(g[:0], 1.0, 1.0, *ok)
    assert torch.equal(g, torch.ones_like(g)) and int(bufs.counter) == 0, 'a refused call launches nothing'
