"""Test helper: record every call a HIP executor makes into its extension module.

``ExtRecorder`` stands in for ``executor.ext``: it forwards every call to the real extension and
keeps ``[function name, normalised args, normalised kwargs]``. Normalisation keeps what a launch
sequence *is* and drops what changes from run to run:

* a tensor becomes ``['T', dtype, shape, ptr-id]``;
* an int >= ``PTR_MIN`` is a device (or host) address and becomes ``['P', ptr-id]``;
* a ptr-id numbers the distinct address values in the order they first appear in the trace, so which
  arguments alias which is kept and the addresses are not;
* floats, bools, None, strings and small ints stay verbatim; lists and tuples are normalised
  recursively.

``record_steps`` builds one of the named learner configurations eagerly and records two consecutive
learner steps (the second consumes the presampled minibatch and the pending hand-offs of the first).
"""
import json
import os

import torch

PTR_MIN = 2 ** 40          # ROCm maps device memory far above this; no count, size or flag comes near it
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'launch_traces')
REPLAY = 4096

RAINBOW = '--dueling --double_dqn --distributional --noisy --prioritized_replay --optimizer=adam'
# name -> (preset, config flags, options)
CONFIGS = {
    'nature_bf16': ('nature', '--dtype=bf16', {}),
    'nature_bf16_det_wgrad': ('nature', '--dtype=bf16 --det_wgrad=1', {}),
    'nature_bf16_no_fuse_wgrad_update': ('nature', '--dtype=bf16 --fuse_wgrad_update=0', {}),
    'nature_bf16_no_fuse_fc_wgrad': ('nature', '--dtype=bf16 --fuse_fc_wgrad=0', {}),
    'nature_bf16_chain1': ('nature', '--dtype=bf16 --chain_dgrad=1', {}),
    'nature_bf16_chain2': ('nature', '--dtype=bf16 --chain_dgrad=2', {}),
    'nature_bf16_two_stream': ('nature', '--dtype=bf16', {'two_stream': True}),
    'nature_bf16_b64': ('nature', '--dtype=bf16 --minibatch_size=64', {}),
    'nature_bf16_dd': ('nature', '--dtype=bf16 --dueling --double_dqn --loss=huber', {}),
    'nature_bf16_acting': ('nature', '--dtype=bf16', {'acting': True}),
    'nature_bf16_dp1': ('nature', '--dtype=bf16', {'dp': True}),
    'rainbow_fp16': ('nature', '--dtype=fp16 ' + RAINBOW, {}),
    'nature_fp32': ('nature', '--dtype=fp32', {}),
    'cnn_fp32': ('atari', '--dtype=fp32', {}),
    'cnn_fp32_no_fuse_fc_wgrad': ('atari', '--dtype=fp32 --fuse_fc_wgrad=0', {}),
    'cnn_bf16': ('atari', '--dtype=bf16', {}),
    'cnn_bf16_no_fuse_fc_wgrad': ('atari', '--dtype=bf16 --fuse_fc_wgrad=0', {}),
}


class ExtRecorder:
    def __init__(self, ext):
        self._ext = ext
        self.calls = []
        self._ids = {}

    def _pid(self, addr: int) -> int:
        return self._ids.setdefault(int(addr), len(self._ids))

    def norm(self, v):
        if isinstance(v, torch.Tensor):
            return ['T', str(v.dtype), list(v.shape), self._pid(v.data_ptr())]
        if isinstance(v, bool) or v is None or isinstance(v, (float, str)):
            return v
        if isinstance(v, int):
            return ['P', self._pid(v)] if v >= PTR_MIN else v
        if isinstance(v, (list, tuple)):
            return [self.norm(x) for x in v]
        raise TypeError('launch trace: unexpected argument %r' % (v,))

    def __getattr__(self, name):
        v = getattr(self._ext, name)
        if not callable(v):
            return v

        def call(*args, **kw):
            self.calls.append([name, self.norm(args), {k: self.norm(kw[k]) for k in sorted(kw)}])
            return v(*args, **kw)
        return call


def dumps(calls) -> str:
    """One call per line, so a golden diff points at the launch that changed."""
    return '[\n' + ',\n'.join(json.dumps(c) for c in calls) + '\n]\n'


def record_steps(name: str, ctx=None):
    """The trace of two eager learner steps of configuration ``name`` on cuda:0."""
    from dist_dqn_amd.config import preset
    from dist_dqn_amd.learner import Learner
    from dist_dqn_amd.models.network import Network
    from dist_dqn_amd.replay import DeviceReplay
    pre, flags, opts = CONFIGS[name]
    dev = torch.device('cuda', 0) if ctx is None else ctx.device
    cfg = preset(pre, 'Pong-v0', '--seed=0 --backend=hip --replay_memory_capacity=%d %s' % (REPLAY, flags))
    net = Network.create_network(cfg, (84, 84, 4), 6, device=dev)
    rep = DeviceReplay(REPLAY, (84, 84), 4, device=dev, prioritized=cfg.prioritized_replay, seed=3)
    rep.fill_synthetic(REPLAY, 6, seed=3)
    ex = net.executor
    if opts.get('two_stream'):
        ex.two_stream = True
    actor = None
    if opts.get('acting'):
        from dist_dqn_amd.actors.device_actor import DeviceActor
        actor = DeviceActor(net, rep, cfg, num_envs=4, steps_per_call=1, seed=11)
        assert actor.can_fuse(cfg.minibatch_size)
    ln = Learner(net, rep, cfg, ctx, use_graph=False, actor=actor)
    if opts.get('dp'):
        assert ln._dp_fused and ln._split and ln._lowrank is not None and ln._defer_fc, 'not the fused DP step'
    # the rule that tells addresses from numbers holds for every buffer and every count we know of
    known = [net.online.flat, net.target.flat, net.grad, rep.frames] + list(net.optimizer.slots)
    assert all(t.data_ptr() >= PTR_MIN for t in known), [hex(t.data_ptr()) for t in known]
    assert max(net.grad.numel() * 4, rep.frames.numel(), 1 << 30) < PTR_MIN
    rec = ExtRecorder(ex.ext)
    ex.ext = rec
    try:
        for _ in range(2):
            ln.step()
        torch.cuda.synchronize(dev)
    finally:
        ex.ext = rec._ext
    assert torch.isfinite(ln.loss).all()
    return rec.calls


def dp_worker(name, port, out_path, errq):
    """Child process of the one-rank data-parallel configuration (a process group of its own)."""
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'DQN_DIST_BACKEND'):
            os.environ.pop(k, None)
        import torch.distributed as dist
        from dist_dqn_amd.config import preset
        from dist_dqn_amd.parallel import init_distributed
        pre, flags, _ = CONFIGS[name]
        cfg = preset(pre, 'Pong-v0', '--seed=0 --backend=hip --replay_memory_capacity=%d %s' % (REPLAY, flags))
        ctx = init_distributed(cfg, device='cuda', force_dp=True)
        assert ctx.enabled and ctx.world_size == 1
        with open(out_path, 'w') as f:
            f.write(dumps(record_steps(name, ctx)))
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        import traceback
        errq.put('%s\n%s' % (e, traceback.format_exc()))
        raise
