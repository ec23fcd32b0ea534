"""The fused fc forward + scalar head launch (csrc/kernels/fc_head.hip) at the shapes where its
tiling changes path, against the separate fc igemm launch + head_loss_kernel on the same net and
minibatch -- the method and the tolerances of
``test_fused_fc_gpu.py::test_folded_head_gradient_matches_separate_head``: 5e-3 relative on the
loss, ``2e-2 * max|prio|`` absolute on the priorities, 2e-2 relative norm per gradient tensor.

* batch sizes 1 (one row), 16 (one row group), 17 (a ragged second group), 32 (two full groups),
  48 (three groups);
* action counts with a template instance (2, 6, 18) and without one (5: the run-time ``A`` path);
* plain, dueling + double (B = 32 with 18 actions: 384 blocks, the two-blocks-per-CU instance;
  B = 48: 576 blocks, more than can be resident, so the tails write the whole dH) and Huber heads;
* every folded case is called twice: ``dh`` and ``dq16`` bit-equal, the row-group counters zero;
* the fp32 build at B = 17, dueling, at the fp32 tolerances of ``test_executor_gpu.py`` (1e-4 on
  the loss and the priorities, 2e-3 per gradient tensor: summation order only);
* fused acting (4 envs, built as ``tests/launch_trace.py`` builds ``nature_bf16_acting``): the
  unfolded head kernel acts in its launch as well, so the folded step's appended actions, rewards
  and dones and the replay cursor are compared with the same two steps run with
  ``fold_head=False``.

(The launch keeps no scratch in the partial-Q buffer beyond each tile's own slot, which every
launch rewrites, so there is no 18-actions-then-2 aliasing case to test.)
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


def _grad(extra, B, A, fold, dtype='bf16'):
    from dist_dqn_amd.config import preset
    from dist_dqn_amd.models.network import Network
    cfg = preset('nature', 'Pong-v0', '--seed=3 --backend=hip --dtype=%s --minibatch_size=%d %s' % (dtype, B, extra))
    net = Network.create_network(cfg, (84, 84, 4), A, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(4)
    net.online.flat.normal_(0.0, 0.03, generator=g)
    net.target.flat.normal_(0.0, 0.03, generator=g)
    net.refresh_packed()
    batch = {
        'states': torch.randint(0, 256, (B, 84, 84, 4), dtype=torch.uint8, device=DEV, generator=g),
        'next_states': torch.randint(0, 256, (B, 84, 84, 4), dtype=torch.uint8, device=DEV, generator=g),
        'actions': torch.randint(0, A, (B,), dtype=torch.int32, device=DEV, generator=g),
        'rewards': torch.randn(B, device=DEV, generator=g) * 5.0,
        'dones': (torch.rand(B, device=DEV, generator=g) < 0.2).float(),
        'gammas': torch.full((B,), 0.99, device=DEV),
    }
    ex = net.executor
    ex.fold_head = fold
    assert ex.can_fold_head(B) == fold
    grad = torch.zeros_like(net.online.flat)
    loss, prio = ex.loss_and_grad(net.online.flat, net.target.flat, batch, grad, None, None)
    torch.cuda.synchronize()
    out = (float(loss), prio.clone(), grad.clone(), net.layout)
    if fold:
        # a repeated call is bit-identical and the launch leaves its row-group counters zero
        ws, fw = ex._workspace(B, DEV), ex._fold_ws(B, DEV)
        assert not fw['cnt'].any()
        dh, dq = ws['dh'][:B * ex.HH].clone(), ws['dq16'][:B * 64].clone()
        grad2 = torch.zeros_like(grad)
        loss2, prio2 = ex.loss_and_grad(net.online.flat, net.target.flat, batch, grad2, None, None)
        torch.cuda.synchronize()
        assert not fw['cnt'].any()
        assert float(loss2) == out[0] and torch.equal(prio2, out[1])
        assert torch.equal(ws['dh'][:B * ex.HH], dh) and torch.equal(ws['dq16'][:B * 64], dq)
        assert ex.fold_errors() == []
    return out


def _compare(extra, B, A, dtype, tol_loss, tol_prio, tol_grad):
    (la, pa, ga, lay), (lb, pb, gb, _) = [_grad(extra, B, A, fold, dtype) for fold in (True, False)]
    print('loss %r vs %r; max |dprio| %.3g of %.3g' % (la, lb, float((pa - pb).abs().max()), float(pb.abs().max())))
    assert abs(la - lb) / abs(lb) < tol_loss, (la, lb)
    torch.testing.assert_close(pa, pb, rtol=0, atol=tol_prio * float(pb.abs().max()))
    for n in lay.names:
        o, k = lay.offsets[n], lay.numel(n)
        x, y = ga[o:o + k].double(), gb[o:o + k].double()
        rel = float((x - y).norm() / (y.norm() + 1e-30))
        assert rel < tol_grad, (n, rel)


DD = '--dueling --double_dqn'


@pytest.mark.parametrize('extra,B,A', [
    ('', 1, 6), ('', 16, 6), ('', 17, 6), ('', 32, 6), ('', 48, 6),          # row groups
    ('', 17, 2), ('', 32, 18), ('', 17, 5),                                  # action counts
    (DD, 17, 6), (DD, 32, 18), (DD, 48, 6), (DD, 16, 2),                     # dueling + double
    ('--loss=huber', 17, 6), (DD + ' --loss=huber', 32, 5),                  # Huber
])
def test_folded_head_matches_separate_head_at_shape(extra, B, A):
    _compare(extra, B, A, 'bf16', 5e-3, 2e-2, 2e-2)


def test_folded_head_matches_separate_head_fp32():
    """fp32 build: both paths compute in fp32, only the summation order differs."""
    _compare('--dueling', 17, 6, 'fp32', 1e-4, 1e-4, 2e-3)


def _acting_steps(fold):
    from dist_dqn_amd.actors.device_actor import DeviceActor
    from dist_dqn_amd.config import preset
    from dist_dqn_amd.learner import Learner
    from dist_dqn_amd.models.network import Network
    from dist_dqn_amd.replay import DeviceReplay
    cfg = preset('nature', 'Pong-v0', '--seed=0 --backend=hip --replay_memory_capacity=4096 --dtype=bf16 '
                 '--fold_head=%d' % int(fold))
    net = Network.create_network(cfg, (84, 84, 4), 6, device=DEV)
    rep = DeviceReplay(4096, (84, 84), 4, device=DEV, prioritized=cfg.prioritized_replay, seed=3)
    rep.fill_synthetic(4096, 6, seed=3)
    actor = DeviceActor(net, rep, cfg, num_envs=4, steps_per_call=1, seed=11)
    assert actor.can_fuse(cfg.minibatch_size)
    ln = Learner(net, rep, cfg, use_graph=False, actor=actor)
    assert net.executor.can_fold_head(cfg.minibatch_size, 4) == fold
    before = rep.cursor.clone()
    for _ in range(2):
        ln.step()
    torch.cuda.synchronize()
    assert net.executor.fold_errors() == []
    return before, rep.cursor.clone(), rep.actions.clone(), rep.rewards.clone(), rep.dones.clone(), float(ln.loss)


def test_folded_head_fused_acting_matches_separate_head():
    """Two learner steps with 4 fused device actors: the actors' decisions and replay appends of
    the folded launch equal those of the unfolded head kernel, which acts in its launch too."""
    b0, c0, a0, r0, d0, l0 = _acting_steps(True)
    b1, c1, a1, r1, d1, l1 = _acting_steps(False)
    assert torch.equal(b0, b1)
    assert not torch.equal(c0, b0), 'the actors appended nothing'
    assert torch.equal(c0, c1), (c0, c1)
    assert torch.equal(a0, a1), (a0 != a1).nonzero().flatten()
    assert torch.equal(r0, r1) and torch.equal(d0, d1)
    assert abs(l0 - l1) / abs(l1) < 5e-3, (l0, l1)
