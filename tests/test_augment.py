"""``--augment shift`` (DrQ random shift) on the CPU: the flags, the torch definition
(``dist_dqn_amd/ops/augment.py``) against a plain numpy loop over the exact Philox replica of
``tests/philox_ref.py``, and a CPU learner step.

The definition (one for the kernel, the torch path and these tests): for minibatch position b and
which in {0: s, 1: s'}, r = philox(seed ^ 0x6175676d, ctr, b, which), dy = (r.x (2P + 1) >> 32) - P,
dx likewise from r.y, out[b, y, x, c] = in[b, clamp(y + dy), clamp(x + dx), c].
"""
import numpy as np
import pytest
import torch

import philox_ref as pr

AUG_KEY = 0x6175676d
SEED = 0x1234567 ^ (5 << 40)
# P = 4, B = 64: over these counters every shift -4..4 occurs on both axes (checked on the replica alone,
# test_reference_counters_cover_every_shift)
COVER_CTRS = list(range(8))


def shifts_ref(seed, ctr, B, pad):
    """int64 [B, 2, 2] of (dy, dx), from the numpy Philox replica."""
    b, which = np.meshgrid(np.arange(B), np.arange(2), indexing='ij')
    x, y, _, _ = pr.philox(int(seed) ^ AUG_KEY, ctr, b, which)
    span = np.uint64(2 * pad + 1)
    dy = ((x * span) >> np.uint64(32)).astype(np.int64) - pad
    dx = ((y * span) >> np.uint64(32)).astype(np.int64) - pad
    return np.stack([dy, dx], axis=-1)


def shift_ref(x, dydx):
    """x [B, H, W, C] -> the shifted stack, one pixel at a time."""
    B, H, W, _ = x.shape
    out = np.empty_like(x)
    for b in range(B):
        dy, dx = int(dydx[b, 0]), int(dydx[b, 1])
        for y in range(H):
            sy = min(max(y + dy, 0), H - 1)
            for xx in range(W):
                out[b, y, xx] = x[b, sy, min(max(xx + dx, 0), W - 1)]
    return out


# ------------------------------------------------------------------------ flags
def test_flags_parse_and_default_off():
    from dist_dqn_amd.config import Config, defaults, parse_args, preset
    d = defaults()
    assert d.augment == 'none' and d.aug_pad == 4
    assert Config().augment == 'none' and Config().aug_pad == 4
    cfg = preset('nature', 'Pong-v0', '--augment shift --aug_pad 7')
    assert cfg.augment == 'shift' and cfg.aug_pad == 7
    assert parse_args(['--network=cnn', '--augment=shift', '--aug_pad=16']).aug_pad == 16
    assert parse_args(['--network=cnn', '--augment=shift', '--aug_pad=1']).aug_pad == 1


@pytest.mark.parametrize('argv', [
    ['--network=nature', '--augment=shift', '--aug_pad=0'],
    ['--network=nature', '--augment=shift', '--aug_pad=17'],
    ['--network=nature', '--augment=flip'],
    ['--network=simple', '--augment=shift'],                     # vector observations
    ['--network=nature', '--augment=shift', '--fuse_sampling=1'],   # the trunk would sample too late
])
def test_flag_errors(argv, capsys):
    from dist_dqn_amd.config import parse_args
    with pytest.raises(SystemExit):
        parse_args(argv)
    assert 'aug' in capsys.readouterr().err


def test_learner_refuses_vector_observations():
    """(A Config built without parse_args: the learner itself checks.)"""
    from dist_dqn_amd.config import parse_args
    from dist_dqn_amd.learner import Learner
    from dist_dqn_amd.models.network import Network
    from dist_dqn_amd.replay import DeviceReplay
    cfg = parse_args(['--device=cpu', '--network=simple', '--minibatch_size=4']).replace(augment='shift')
    net = Network.create_network(cfg, (4,), 2)
    rep = DeviceReplay(64, (4,), 1, device='cpu')
    with pytest.raises(ValueError, match='image observations'):
        Learner(net, rep, cfg)


# ------------------------------------------------------------------ definition
def test_torch_philox_equals_the_numpy_replica():
    from dist_dqn_amd.ops import augment
    lo0 = np.arange(70).reshape(-1, 1)
    lo1 = np.array([0, 1, 0x6e6f6973, 2 ** 32 - 1]).reshape(1, -1)
    for key, ctr in [(0, 0), (SEED ^ AUG_KEY, 5), (2 ** 64 - 1, 2 ** 64 - 1), (0x9E3779B97F4A7C15, 2 ** 32 + 3)]:
        want = pr.philox(key, ctr, lo0, lo1)
        c = ctr if ctr < 2 ** 63 else ctr - 2 ** 64
        for ctr_arg in (ctr, torch.tensor([c], dtype=torch.int64)):
            got = augment.philox(key, ctr_arg, torch.from_numpy(lo0), torch.from_numpy(lo1))
            for g, w in zip(got, want):
                assert np.array_equal(g.numpy().astype(np.uint64), w), (key, ctr)


@pytest.mark.parametrize('pad', [1, 4, 16])
def test_shift_stacks_equals_numpy_loop(pad):
    from dist_dqn_amd.ops import augment
    B, H, W = 3, 84, 84
    g = np.random.default_rng(pad)
    s = g.integers(0, 256, (B, H, W, 4), dtype=np.uint8)
    ns = g.integers(0, 256, (B, H, W, 4), dtype=np.uint8)
    for ctr in (0, 7, 2 ** 32 + 11):
        sh = shifts_ref(SEED, ctr, B, pad)
        assert sh.min() >= -pad and sh.max() <= pad
        for ctr_arg in (ctr, torch.tensor([ctr], dtype=torch.int64)):
            a, b, got = augment.shift_stacks(torch.from_numpy(s), torch.from_numpy(ns), SEED, ctr_arg, pad)
            assert got.dtype == torch.int64 and np.array_equal(got.numpy(), sh)
            assert a.dtype == torch.uint8 and a.is_contiguous() and tuple(a.shape) == (B, H, W, 4)
            assert np.array_equal(a.numpy(), shift_ref(s, sh[:, 0]))
            assert np.array_equal(b.numpy(), shift_ref(ns, sh[:, 1]))


def test_reference_counters_cover_every_shift():
    """P = 4 at B = 64 over COVER_CTRS: every value in -4..4 occurs on both axes, for s and for s'
    (on the replica alone; the torch path draws the same values)."""
    from dist_dqn_amd.ops import augment
    sh = np.stack([shifts_ref(SEED, c, 64, 4) for c in COVER_CTRS])        # [ctr, B, which, axis]
    for which in range(2):
        for axis in range(2):
            assert set(np.unique(sh[:, :, which, axis]).tolist()) == set(range(-4, 5)), (which, axis)
    for c in COVER_CTRS:
        assert np.array_equal(augment.draw_shifts(SEED, c, 64, 4).numpy(), shifts_ref(SEED, c, 64, 4))
    # s and s' draw independently, and consecutive steps draw afresh
    assert not np.array_equal(sh[0, :, 0], sh[0, :, 1]) and not np.array_equal(sh[0], sh[1])


def test_seed_and_rank_change_the_stream():
    from dist_dqn_amd.ops import augment
    seeds = {augment.aug_seed(s, r) for s in (None, 0, 1, 7) for r in (0, 1, 2)}
    assert len(seeds) == 9 and augment.aug_seed(None) == augment.aug_seed(0)     # (no --seed: seed 0)
    assert all(0 <= s < 2 ** 63 for s in seeds)
    a = augment.draw_shifts(augment.aug_seed(3, 0), 0, 64, 4)
    assert not torch.equal(a, augment.draw_shifts(augment.aug_seed(3, 1), 0, 64, 4))
    assert torch.equal(a, augment.draw_shifts(augment.aug_seed(3, 0), 0, 64, 4))


def test_cpu_gather_shift_wrapper_matches_the_definition():
    """ops.kernels.replay_gather_shift on CPU tensors: gather through the slot tables, then the shift;
    pad = 0 is the plain gather."""
    from dist_dqn_amd.ops import kernels
    g = np.random.default_rng(0)
    frames = g.integers(0, 256, (9, 84, 84), dtype=np.uint8)
    st = g.integers(0, 9, (3, 4)).astype(np.int32)
    nx = g.integers(0, 9, (3, 4)).astype(np.int32)
    stack = lambda sl: np.stack([frames[sl[:, c]] for c in range(4)], axis=-1)
    ctr = torch.tensor([3], dtype=torch.int64)
    s, ns, sh = kernels.replay_gather_shift(torch.from_numpy(frames), torch.from_numpy(st), torch.from_numpy(nx),
                                            SEED, ctr, 4)
    want = shifts_ref(SEED, 3, 3, 4)
    assert sh.dtype == torch.int32 and np.array_equal(sh.numpy(), want)
    assert np.array_equal(s.numpy(), shift_ref(stack(st), want[:, 0]))
    assert np.array_equal(ns.numpy(), shift_ref(stack(nx), want[:, 1]))
    s0, ns0, sh0 = kernels.replay_gather_shift(torch.from_numpy(frames), torch.from_numpy(st), torch.from_numpy(nx),
                                               SEED, ctr, 0)
    assert np.array_equal(s0.numpy(), stack(st)) and np.array_equal(ns0.numpy(), stack(nx)) and not sh0.any()


# ------------------------------------------------------------------ learner step
def _cpu_learner(extra, seed=5):
    from dist_dqn_amd.config import parse_args
    from dist_dqn_amd.learner import Learner
    from dist_dqn_amd.models.network import Network
    from dist_dqn_amd.replay import DeviceReplay
    cfg = parse_args(['--device=cpu', '--seed=%d' % seed, '--network=cnn', '--optimizer=rmsprop', '--minibatch_size=4',
                      '--replay_memory_capacity=64', '--lr=0.01'] + extra)
    net = Network.create_network(cfg, (84, 84, 4), 6)
    rep = DeviceReplay(64, (84, 84), 4, device='cpu', seed=0)
    rep.fill_synthetic(64, 6, seed=0, episode_len=16)
    return cfg, net, rep, Learner(net, rep, cfg)


def test_cpu_learner_step_augments_and_is_reproducible():
    """Same weights, same minibatch: the augmented step's loss and parameters differ from the plain
    step's, equal a second augmented run's bit for bit, and follow the seed; the step consumed exactly the
    reference shifts of (aug_seed(seed, rank 0), global_step 0), then of global_step 1."""
    from dist_dqn_amd.ops import augment
    runs = {}
    for name, extra, seed in [('plain', [], 5), ('aug', ['--augment=shift'], 5), ('aug2', ['--augment=shift'], 5),
                              ('other', ['--augment=shift'], 6)]:
        cfg, net, rep, ln = _cpu_learner(extra, seed)
        if name == 'other':       # the other seed's net differs anyway: compare the drawn shifts
            ln.step()
            runs[name] = ln.aug_shifts.clone()
            continue
        l0 = float(ln.step())
        sh0 = ln.aug_shifts.clone() if ln.aug_shifts is not None else None
        l1 = float(ln.step())
        runs[name] = (l0, l1, net.online.flat.clone(), sh0, ln.aug_shifts)
    plain, aug, aug2 = runs['plain'], runs['aug'], runs['aug2']
    assert plain[3] is None and plain[4] is None
    assert aug[0] != plain[0] and not torch.equal(aug[2], plain[2])
    assert aug[0] == aug2[0] and aug[1] == aug2[1] and torch.equal(aug[2], aug2[2])
    s = augment.aug_seed(5, 0)
    assert np.array_equal(aug[3].numpy(), shifts_ref(s, 0, 4, 4)) and np.array_equal(aug[4].numpy(), shifts_ref(s, 1, 4, 4))
    assert np.abs(aug[3].numpy()).max() > 0
    assert not torch.equal(runs['other'], aug[3])
