"""Every built native-extension variant (bf16 _C, fp16 _C_f16, fp32 _C_f32) imports, alone and
all together in one process (module-local pybind types; -Bsymbolic kernel launchers)."""
import importlib
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _built(name):
    pkg = os.path.join(ROOT, 'dist_dqn_amd')
    return any(f.startswith(name + '.') and f.endswith('.so') for f in os.listdir(pkg))


def test_all_variants_import_together():
    names = [n for n in ('_C', '_C_f16', '_C_f32') if _built(n)]
    if not names:
        pytest.skip('native extension not built')
    mods = [importlib.import_module('dist_dqn_amd.' + n) for n in names]
    for m in mods:
        assert hasattr(m, 'qnet_igemm') and hasattr(m, 'optim_pack') and hasattr(m, 'InferServer')


def test_ingest_server_binding_converts_lists():
    """The Ape-X ingest thread's constructor takes Python lists (pybind11 STL casters): a call
    with wrong list sizes must reach the C++ argument check, not fail the type conversion."""
    if not _built('_C'):
        pytest.skip('native extension not built')
    m = importlib.import_module('dist_dqn_amd._C')
    with pytest.raises(RuntimeError, match='argument sizes'):
        m.IngestServer(0, 1, 0, 4, 0.99, [0] * 7, [0] * 4, [0] * 3, [0] * 11, 0)


# csrc/include/dqn_kernels.h launch_optim_pack (extern "C++": the Itanium-mangled name of its signature)
_LAUNCH_OPTIM_PACK = ('_Z17launch_optim_packiPfPKfS_S_S_PlPiS1_ffifPKviPvS_S6_iiS1_S_S1_S_iPKN3dqn11TrunkSampleEPK7PerStep'
                      'S1_S_S6_S2_PK6FcFuseS1_S5_iS5_S6_iP12ihipStream_t')


@pytest.mark.parametrize('name', ['_C', '_C_f16', '_C_f32'])
def test_optim_pack_launcher_refuses_unbuilt_modes(name):
    """``launch_optim_pack`` called directly (the binding's own argument checks refuse these
    combinations earlier, so Python cannot reach this through ``ext.optim_pack``): a target mix
    without noise is mode 2, which optim_pack.h DQN_OPT_MODES does not list, on the few-block
    table (no jobs) and on the main table (> 256 jobs); so is an optimizer op that does not exist.
    Each returns false before any kernel is enqueued -- the call needs no GPU, and every device
    pointer it is given is null or never dereferenced."""
    import ctypes as C
    if not _built(name):
        pytest.skip('native extension not built')
    lib = C.CDLL(importlib.import_module('dist_dqn_amd.' + name).__file__)
    assert hasattr(lib, _LAUNCH_OPTIM_PACK), 'launch_optim_pack: signature changed, update the mangled name'
    P, I, F = C.c_void_p, C.c_int, C.c_float
    fn = getattr(lib, _LAUNCH_OPTIM_PACK)
    fn.restype = C.c_bool
    fn.argtypes = [I] + [P] * 8 + [F, F, I, F, P, I, P, P, P, I, I, P, P, P, P, I] + [P] * 9 + [I, P, P, I, P]
    hp9 = (C.c_float * 9)()

    def launch(op, njobs, tnoise):
        # op, w g s0 s1 beta_pow step ticket, hp9, lr reg reg_end grad_scale, jobs njobs, packed tgt tgt_packed,
        # tfreq max_grid, noise eff gnoise noise_dst noise_n, smp per, tnoise teff tpk noise_rng fc part wg,
        # wg_blocks, dp tsg, no_pack, stream
        return fn(op, *[None] * 7, C.cast(hp9, P), 0.1, 0.0, 0, 1.0, None, njobs, None, None, None, 1, 2048,
                  None, None, None, None, 0, None, None, tnoise, None, None, None, None, None, None, 0, None, None, 0,
                  None)

    assert launch(0, 0, 16) is False         # RMSProp-class op 0, few-block table (16-bit builds)
    assert launch(0, 300, 16) is False       # main table
    assert launch(1, 0, 16) is False         # an optimizer without few-block variants
    assert launch(99, 0, None) is False      # no such optimizer
