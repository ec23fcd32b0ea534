"""End-to-end learning with --max_grad_norm 10 on the HIP learner (GPU): the `nature` net on the
BlockBandit task of test_learning_gpu.py, with test_qr_learning_gpu.py's step budget and pass
criterion (reward 1 for naming the band of the bright block in the newest frame; random play
scores episode_len / A)."""
import numpy as np
import pytest

from test_learning_gpu import _episode_rewards

pytestmark = pytest.mark.gpu


def test_hip_clipped_learner_learns_block_bandit(tmp_path):
    from dist_dqn_amd.cli import run_worker
    from dist_dqn_amd.config import preset
    cfg = preset('nature', 'SyntheticBlock-v0',
                 '--seed=0 --device=cuda --backend=hip --dtype=bf16 --replay_memory_capacity=20000 '
                 '--replay_start_size=500 --update_freq=1 --target_update_freq=200 '
                 '--random_action_explore_steps=2000 --min_random_action_prob=0.05 --reward_discount=0.9 '
                 '--max_steps_per_episode=8 --num_episodes=100000 --max_train_steps=2500 '
                 '--max_grad_norm=10 --checkpoint_secs=0 --logdir=%s' % tmp_path)
    agent = run_worker(cfg)
    assert agent.network.executor.name.startswith('hip')
    assert agent.training_steps == 2500
    ln = agent.session
    assert ln._clip == 10.0 and not ln._defer_fc and not ln._defer_wgrad
    gn = float(ln.grad_norm)
    assert np.isfinite(gn) and gn > 0.0, gn
    r = _episode_rewards(str(tmp_path))
    chance = 8.0 / 4
    first, last = np.mean(r[:50]), np.mean(r[-100:])
    print('clipped nature: first-50 mean %.2f, last-100 mean %.2f (chance %.2f, max 8), last grad_norm %.4g'
          % (first, last, chance, gn))
    assert last > 2.0 * chance and last > first + 1.0, (first, last)
