"""Launch-trace characterisation of the fused executor: the sequence of extension calls two eager
learner steps make, argument by argument (addresses replaced by aliasing ids, ``launch_trace.py``),
against the goldens in ``tests/golden/launch_traces``. The configurations are the smallest that reach
every branch of ``HipExecutor.loss_and_grad`` / ``update_and_pack``; a structural change of those
methods that launches the same work leaves every golden unchanged.

``DQN_RECORD_TRACES=1`` writes the goldens instead of comparing (record on the commit whose behaviour
is to be kept, twice, and check that the two recordings are byte-identical). The goldens here were
recorded that way on the executor as it stood before its step was split into phases: this module
and ``launch_trace.py`` use only the public learner and ``executor.ext``, so they run unchanged on
that older tree, which is how to re-record or re-check them.
"""
import multiprocessing as mp
import os
import socket

import pytest

import launch_trace as lt

pytestmark = pytest.mark.gpu


def _dp_trace(name, tmp_path) -> str:
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    errq = ctx.SimpleQueue()
    out = str(tmp_path / 'trace.json')
    p = ctx.Process(target=lt.dp_worker, args=(name, port, out, errq))
    p.start()
    p.join(timeout=150)
    if p.is_alive():
        p.kill()
        pytest.fail('the one-rank data-parallel learner hung')
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not errs and p.exitcode == 0, '\n'.join(errs) or p.exitcode
    with open(out) as f:
        return f.read()


@pytest.mark.parametrize('name', sorted(lt.CONFIGS))
def test_launch_trace_matches_golden(name, tmp_path):
    got = _dp_trace(name, tmp_path) if lt.CONFIGS[name][2].get('dp') else lt.dumps(lt.record_steps(name))
    path = os.path.join(lt.GOLDEN_DIR, name + '.json')
    if os.environ.get('DQN_RECORD_TRACES') == '1':
        os.makedirs(lt.GOLDEN_DIR, exist_ok=True)
        with open(path, 'w') as f:
            f.write(got)
        return
    assert os.path.exists(path), 'no golden trace for %s (record it with DQN_RECORD_TRACES=1)' % name
    with open(path) as f:
        want = f.read()
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        i = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        pytest.fail('%s: %d calls recorded, %d in the golden; first difference at line %d:\n got  %s\n want %s'
                    % (name, len(g) - 2, len(w) - 2, i + 1, g[i] if i < len(g) else '<end>',
                       w[i] if i < len(w) else '<end>'))
