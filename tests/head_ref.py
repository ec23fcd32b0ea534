"""Test helper: the harness the rows heads' tests share (test_c51_head_gpu.py, test_qr_head_gpu.py,
test_qr_wide_head_gpu.py, test_munchausen_head_gpu.py). A rows head reads precomputed fp32 output
rows [B][KD] by pointer, so its kernels run on synthetic rows with no network. Each head's file
keeps what is its own: the row layout, the seeded inputs, the float64 reference, the error bound
and its derivation, the cases. Here is what they do alike: the replay-batch columns of the inputs,
the sentinel-filled launches, and every assertion on a training launch's outputs.
"""
import numpy as np
import torch

DEV = torch.device('cuda', 0)
SENT = -4096.0                 # exact in bf16 / fp16 / fp32, below anything the kernels can write
PAD_IN = 1e9                   # the input rows' pad columns: a kernel that read one would show it
HID = 128                      # (unused by the rows heads' kernels; the bindings want a multiple of 128)
E24 = 2.0 ** -24
# variant -> (act_t as HipExecutor.act_dtype maps it, storage rounding step, kLossScale)
BUILDS = {'': (torch.bfloat16, 2.0 ** -8, 1.0), 'f16': (torch.float16, 2.0 ** -11, 1024.0),
          'f32': (torch.float32, 0.0, 1.0)}


def dims(A, N, dueling):
    """(NO, VO, KD) of rows [A * N outputs | pad | N dueling value outputs at VO | pad]."""
    NO = A * N
    VO = (NO + 31) // 32 * 32
    return NO, VO, VO + ((N + 31) // 32 * 32 if dueling else 0)


def ext(variant):
    from dist_dqn_amd.ops import _ext as loader
    return loader.load(required=True, variant=variant)


# ------------------------------------------------------------------ inputs (CPU, seeded)
# Each draws from the head's generator when the head's ``_inputs`` calls it: the order of the calls
# is the head's own.
def draw_transitions(g, B, edges, scale=1.0):
    """(rew, done, gam) [B]: normal rewards times ``scale``, a fifth terminal, gamma^(1..3); the
    first rows are the head's edge rows (reward, done, gamma)."""
    rew = torch.randn(B, generator=g) * scale
    done = (torch.rand(B, generator=g) < 0.2).float()
    gam = torch.tensor([0.99 ** (1 + i % 3) for i in range(B)])
    for i, (r, d, gm) in enumerate(edges[:B]):
        rew[i], done[i], gam[i] = r, d, gm
    return rew.float(), done, gam.float()


def draw_actions(g, B, A):
    act = torch.randint(0, A, (B,), generator=g, dtype=torch.int32)
    act[0] = A - 1
    act[B - 1] = 0
    return act


def draw_weights(g, B, wmode):
    """(wts [B] or None, the zero-weight row or None) for wmode 'none' / 'rand' / 'zero'."""
    if wmode == 'none':
        return None, None
    wts, zrow = torch.rand(B, generator=g) + 0.5, None
    if wmode == 'zero':
        zrow = 10 if B > 10 else B - 1
        wts[zrow] = 0.0
    return wts.float(), zrow


# ------------------------------------------------------------------ launches
def _call(ext, fn_name, ints, dist, flts, io, lg, qp):
    prof = [0] if fn_name == 'qnet_c51_head' else []          # (the C51 binding's positional prof)
    getattr(ext, fn_name)(ints, dist, flts, [], [], [], [], [], io, [], [], [], [], [], *prof, lg, 0, qp)
    torch.cuda.synchronize()


def train(ext, fn_name, ints, dist, flts, c, act_t, ninst, KD):
    """One training launch on case ``c`` with sentinel-filled outputs of 8 rows (loss partials: 8
    entries) more than the launch may write: (dout [(B + 8) * KD], prio [B + 8], parts [72])."""
    B = ints[0]
    t = {k: c[k].to(DEV).contiguous() for k in ('rows', 'rew', 'done', 'gam', 'act')}
    wts = None if c['wts'] is None else c['wts'].to(DEV)
    dout = torch.full(((B + 8) * KD,), SENT, dtype=act_t, device=DEV)
    prio = torch.full((B + 8,), SENT, dtype=torch.float32, device=DEV)
    parts = torch.full((72,), SENT, dtype=torch.float32, device=DEV)
    io = [t['act'].data_ptr(), t['rew'].data_ptr(), t['done'].data_ptr(), t['gam'].data_ptr(),
          0 if wts is None else wts.data_ptr(), 0, prio.data_ptr()] + [0] * 6
    _call(ext, fn_name, ints, dist, flts, io, [t['rows'][i].data_ptr() for i in range(ninst)],
          [parts.data_ptr(), dout.data_ptr()])
    return dout.cpu(), prio.cpu(), parts.cpu()


def infer(ext, fn_name, dist, flts, rows, B, A, dueling):
    """The q_values launch on rows [B][KD]: Q [B, A] as float64, exactly [B][A] written."""
    r = rows.to(DEV).contiguous()
    q = torch.full((B * A + 8,), float('nan'), dtype=torch.float32, device=DEV)
    _call(ext, fn_name, [B, A, HID, int(dueling), 0, 1], dist, flts, [0] * 7 + [q.data_ptr()] + [0] * 5,
          [r.data_ptr()], [])
    q = q.cpu()
    assert torch.isnan(q[B * A:]).all(), 'written beyond [B][A]'
    assert not torch.isnan(q[:B * A]).any(), 'q_out left unwritten'
    return q[:B * A].double().numpy().reshape(B, A)


def check_train(variant, c, call, ninst, KD, nb, ref, words, ratios, rel=0.0):
    """Two training launches of build ``variant`` on case ``c`` against the head's float64 reference.
    call = (fn_name, ints, dist, flts); nb = the learner blocks (= loss partials) of the launch;
    ref: ``g`` [B, KD] the dZ rows before the w / B factor, ``t`` [B, KD] the fp32 error bound of
    ``g``, ``mask`` [KD] the written columns, ``prio`` [B] the priorities, ``per`` [B] the per-sample
    loss, ``w`` [B] the weights, ``skip`` [B] the near-tie rows left out (their ``prio`` is ``per``)
    or None; rel: relative fp32 error of the dZ rows on top of the storage rounding;
    words = (the priority's label, its symbol, the written columns' name);
    ratios: the file's {variant: largest err / bound so far}."""
    act_t, ulp, scale = BUILDS[variant]
    B = c['B']
    g, t, mask, w = ref['g'], ref['t'], ref['mask'], ref['w']
    keep = np.ones(B, dtype=bool) if ref['skip'] is None else ~ref['skip']
    assert int((~keep).sum()) * 16 <= B, ('near-ties in the reference: pick another seed', np.nonzero(~keep)[0])
    e = ext(variant)
    dout, prio, parts = train(e, *call, c, act_t, ninst, KD)
    dout2, prio2, parts2 = train(e, *call, c, act_t, ninst, KD)
    assert torch.equal(prio, prio2) and torch.equal(dout.view(torch.uint8), dout2.view(torch.uint8)) \
        and torch.equal(parts, parts2), 'repeatability'
    # layout and write coverage
    d = dout.double().view(B + 8, KD).numpy()
    assert (d[:B][:, ~mask] == SENT).all(), 'a pad column was written'
    assert (d[B:] == SENT).all() and (prio[B:] == SENT).all(), 'a row beyond B was written'
    assert (d[:B][:, mask] != SENT).all() and (prio[:B] != SENT).all(), words[2] + ' was left unwritten'
    assert (parts[nb:] == SENT).all() and (parts[:nb] != SENT).all(), 'loss partials'
    assert np.isfinite(d[:B][:, mask]).all() and torch.isfinite(prio[:B]).all() and torch.isfinite(parts[:nb]).all()
    # priorities and the loss (the fc dgrad launch's aux duty: sum / B)
    pk = prio[:B].double().numpy()
    print('%s: max |err| %.3g at |%s| up to %.3g' % (words[0], np.abs(pk - ref['prio'])[keep].max(), words[1],
                                                    ref['prio'].max()))
    np.testing.assert_allclose(pk[keep], ref['prio'][keep], rtol=1e-4, atol=1e-5)
    loss_ref = float((w * np.where(keep, ref['per'], pk)).sum() / B)
    np.testing.assert_allclose(float(parts[:nb].double().sum()) / B, loss_ref, rtol=1e-4, atol=1e-5)
    # the dZ rows
    wb = (w / B)[:, None]
    want = g * wb * scale
    bound = (ulp + rel) * np.abs(want) + t * wb * scale
    err = np.abs(d[:B] - want)
    sel = keep[:, None] & mask[None, :]
    ratio = np.where(sel & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0)
    ratios[variant] = max(ratios.get(variant, 0.0), float(ratio.max()))
    print('dout16 %r: max err / bound %.3f (build so far %.3f)' % (variant, ratio.max(), ratios[variant]))
    bad = sel & (err > bound)
    assert not bad.any(), (int(bad.sum()), [(int(b), int(k), d[b, k], want[b, k]) for b, k in np.argwhere(bad)[:5]])
    if c['zrow'] is not None:
        assert (d[c['zrow']][mask] == 0.0).all(), 'zero-weight row'
