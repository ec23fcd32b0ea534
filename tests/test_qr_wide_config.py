"""Which QR-DQN quantile counts the HIP executor takes (no GPU): 2..64 on qr_head.hip, 68..256 in
multiples of 4 on qr_wide_head.hip; every other count, and C51 beyond 64 atoms, stays with the
torch executor."""
import pytest


def _arch(argv):
    from dist_dqn_amd.config import parse_args
    from dist_dqn_amd.models.arch import arch_from_config
    return arch_from_config(parse_args(['--network=nature'] + argv), (84, 84, 4), 18)


@pytest.mark.parametrize('n,ok', [(64, True), (68, True), (128, True), (200, True), (256, True),
                                  (65, False), (66, False), (258, False), (260, False), (300, False)])
def test_supports_quantile_counts(n, ok):
    from dist_dqn_amd.ops.executor import supports
    a = _arch(['--quantile', '--num_quantiles=%d' % n, '--dueling', '--double_dqn'])
    assert a.quantile and a.atoms == n and supports(a) is ok


def test_c51_stays_at_64_atoms():
    from dist_dqn_amd.ops.executor import supports
    assert supports(_arch(['--distributional', '--num_atoms=64']))
    assert not supports(_arch(['--distributional', '--num_atoms=128']))


def test_help_names_the_wide_range():
    from dist_dqn_amd.config import build_parser
    text = ' '.join(build_parser().format_help().split())
    assert '2..64' in text and '68..256' in text and 'multiples of 4' in text
