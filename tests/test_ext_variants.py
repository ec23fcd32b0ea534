"""Every built native-extension variant (bf16 _C, fp16 _C_f16, fp32 _C_f32) imports, alone and
all together in one process (module-local pybind types; -Bsymbolic kernel launchers)."""
import ctypes
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


# csrc/include/dqn_kernels.h: bool launch_optim_pack(const OptimPackArgs&, hipStream_t) (extern "C++": the
# Itanium-mangled name of its signature) and OptimPackArgs, field by field
_LAUNCH_OPTIM_PACK = '_Z17launch_optim_packRK13OptimPackArgsP12ihipStream_t'
_P, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


class OptimPackArgs(ctypes.Structure):
    _fields_ = [
        # core buffers and hyper-parameters
        ('op', _I), ('w', _P), ('g', _P), ('s0', _P), ('s1', _P), ('beta_pow', _P), ('step', _P), ('ticket', _P),
        ('hp9', ctypes.POINTER(_F)), ('lr', _F), ('reg', _F), ('reg_end', _I), ('grad_scale', _F),
        # job table and packed output
        ('jobs', _P), ('njobs', _I), ('packed', _P), ('max_grid', _I), ('no_pack', _I), ('part', _P),
        # target
        ('tgt', _P), ('tgt_packed', _P), ('tfreq', _I), ('tsg', _P),
        # noise
        ('noise', _P), ('eff', _P), ('gnoise', _P), ('noise_dst', _P), ('noise_n', _I), ('noise_rng', _P),
        ('tnoise', _P), ('teff', _P), ('tpk', _P),
        # sampler
        ('smp', _P), ('per', _P),
        # fused gradients
        ('fc', _P), ('wg', _P), ('wg_blocks', _I), ('dp', _P),
    ]


@pytest.mark.parametrize('name', ['_C', '_C_f16', '_C_f32'])
def test_optim_pack_launcher_refuses_unbuilt_modes(name):
    """``launch_optim_pack`` called directly (the binding's own argument checks refuse these
    combinations earlier, so Python cannot reach this through ``ext.optim_pack``): a target mix
    without noise is mode 2, which optim_pack.h DQN_OPT_MODES does not list, on the few-block
    table (no jobs) and on the main table (> 256 jobs); so is an optimizer op that does not exist.
    Each returns false before any kernel is enqueued -- the call needs no GPU, and every device
    pointer it is given is null or never dereferenced."""
    if not _built(name):
        pytest.skip('native extension not built')
    mod = importlib.import_module('dist_dqn_amd.' + name)
    assert ctypes.sizeof(OptimPackArgs) == mod.OPTIM_PACK_ARGS_BYTES, 'OptimPackArgs: field list out of step'
    lib = ctypes.CDLL(mod.__file__)
    assert hasattr(lib, _LAUNCH_OPTIM_PACK), 'launch_optim_pack: signature changed, update the mangled name'
    fn = getattr(lib, _LAUNCH_OPTIM_PACK)
    fn.restype = ctypes.c_bool
    fn.argtypes = [ctypes.POINTER(OptimPackArgs), _P]
    hp9 = (_F * 9)()

    def launch(op, njobs, tnoise):
        a = OptimPackArgs()                  # zeroed: everything else absent
        a.op, a.njobs, a.max_grid, a.hp9, a.tnoise = op, njobs, 2048, hp9, tnoise
        return fn(ctypes.byref(a), None)

    assert launch(0, 0, 16) is False         # RMSProp-class op 0, few-block table (16-bit builds)
    assert launch(0, 300, 16) is False       # main table
    assert launch(1, 0, 16) is False         # an optimizer without few-block variants
    assert launch(99, 0, None) is False      # no such optimizer
