"""CPU checks of the evaluation layer: the NumPy restatement of the two kernel contracts (tests/eval_ref.py) against plain
Python loops written from benchmark_agent.py:59-106 and against the reference's own run (tests/golden/eval_n5.npz, written by
tests/golden/gen_eval_golden.py), and `TrainedAgent`'s network-index map (SAC_agents.py:72-75, :88-96)."""
import numpy as np
import pytest

from scalable_collision_avoidance_rl_amd.evaluate import network_index, summarize_evaluation
from tests import eval_ref
from tests.helpers import load


def _loops(w, gamma):
    """benchmark_agent.py:59-106 for every env of a window, one Python loop per env: `while not finished` over the stored
    steps, then benchmark_cirtic's backward recurrence (SAC_agents.py:109-113) over the episode's own rewards."""
    T, E, N = w["reward"].shape
    out = []
    for e in range(E):
        total_episode_reward = total_true_episode_reward = 0.0                     # :59-61
        total_episode_collisions = t_iter = 0
        finished = False
        rewards_seen = []
        while not finished and t_iter < T:                                         # :69
            rewards = w["reward"][t_iter, e].astype(np.float64); true_rewards = w["true_reward"][t_iter, e].astype(np.float64)
            finished = bool(w["done"][t_iter, e])
            total_episode_reward += np.mean(rewards)                               # :85
            total_true_episode_reward += np.mean(true_rewards)                     # :86
            total_episode_collisions += int(w["n_coll"][t_iter, e])                # :87
            rewards_seen.append(rewards)
            t_iter += 1                                                            # :94
        if not finished:                                                           # the window ended first: no episode
            out.append(None)
            continue
        Gt = np.zeros((t_iter, N))                                                 # SAC_agents.py:109-113
        Gt[-1] = rewards_seen[-1]
        for t in range(t_iter - 2, -1, -1):
            Gt[t] = Gt[t + 1] * gamma + rewards_seen[t]
        advantage = [np.mean(Gt[:, i] - w["V"][:t_iter, e, i].astype(np.float64)) for i in range(N)]   # :105
        out.append((total_episode_reward, total_true_episode_reward, total_episode_collisions, t_iter, Gt, advantage))
    return out


@pytest.mark.parametrize("shape", [(1, 1, 2), (7, 3, 2), (40, 11, 5), (23, 6, 8)])
def test_eval_ref_matches_benchmark_agent_loops(shape):
    gamma = 0.97
    w = eval_ref.synthetic_window(*shape, seed=3)
    ref = eval_ref.episode_eval(w["reward"], w["true_reward"], w["n_coll"], w["done"], w["V"], gamma)
    seen_none = seen_some = False
    for e, row in enumerate(_loops(w, gamma)):
        if row is None:
            seen_none = True
            assert ref["ep_len"][e] == 0 and ref["ep_collisions"][e] == 0 and ref["ep_return"][e] == 0
            assert not ref["agent_return"][e].any() and not ref["mean_adv"][e].any() and not ref["agent_true_return"][e].any()
            continue
        seen_some = True
        ret, tret, coll, L, Gt, adv = row
        assert ref["ep_len"][e] == L and ref["ep_collisions"][e] == coll
        np.testing.assert_allclose(ref["ep_return"][e], ret, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ref["ep_true_return"][e], tret, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ref["G"][:L, e], Gt, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ref["mean_adv"][e], adv, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ref["agent_return"][e].mean(), ret, rtol=1e-12, atol=1e-12)
    assert seen_some or shape[1] == 1
    assert seen_none or shape[1] < 5


def test_synthetic_windows_hold_every_done_pattern():
    w = eval_ref.synthetic_window(19, 9, 4, seed=1)
    d = w["done"]
    per_env = d.sum(0)
    assert (per_env == 0).any() and (per_env > 1).any()
    assert d[0].any() and ((per_env == 1) & (d[-1] == 1)).any()
    ref = eval_ref.episode_eval(w["reward"], w["true_reward"], w["n_coll"], d, None, 0.99)
    assert "mean_adv" not in ref and (ref["ep_len"][per_env > 1] < 19).any()


def test_histogram_ref():
    v = np.array([0, 0, 3, 7, 40, -1, 2, 31, 32], np.int32)
    h = eval_ref.histogram(v, 32)
    assert h.shape == (33,) and h.sum() == 8 and h[0] == 2 and h[32] == 2 and h[31] == 1
    h = eval_ref.histogram(v, 4, valid=np.array([1, 0, 1, 1, 1, 1, 1, 0, 1]))
    assert h.tolist() == [1, 0, 1, 1, 3]


def test_eval_ref_reproduces_the_reference_episode():
    """eval_n5.npz: the reference's own totals (benchmark_agent.py:85-87, :94), `benchmark_cirtic`'s Gts and the advantage of
    :105 from its stored tuples, to 1e-12."""
    fx = load("eval_n5.npz")
    T = int(fx["t_iter"])
    assert fx["reward"].shape == (T, 5) and bool(fx["finished"][-1]) and not fx["finished"][:-1].any()
    pad = 3                                   # steps behind the episode's end in the window: they must not count
    rng = np.random.default_rng(0)
    ext = lambda a: np.concatenate([a, rng.standard_normal((pad,) + a.shape[1:])])[:, None]
    done = np.concatenate([fx["finished"], [False, True, False]]).astype(np.uint8)[:, None]
    n_coll = np.concatenate([fx["n_coll"], [5, 5, 5]])[:, None]
    ref = eval_ref.episode_eval(ext(fx["reward"]), ext(fx["true_reward"]), n_coll, done, ext(fx["V_approxs"].astype(np.float64)),
                                float(fx["discount"]))
    assert ref["ep_len"][0] == T and ref["ep_collisions"][0] == int(fx["total_collisions"])
    assert abs(ref["ep_return"][0] - float(fx["total_reward"])) <= 1e-12 * (1 + abs(float(fx["total_reward"])))
    assert abs(ref["ep_true_return"][0] - float(fx["total_true_reward"])) <= 1e-12 * (1 + abs(float(fx["total_true_reward"])))
    assert np.abs(ref["G"][:T, 0] - fx["Gts"]).max() <= 1e-12 * (1 + np.abs(fx["Gts"]).max())
    assert np.abs(ref["mean_adv"][0] - fx["advantage"]).max() <= 1e-12 * (1 + np.abs(fx["advantage"]).max())


def test_network_index_map():
    assert network_index(5, 5) == [0, 1, 2, 3, 4]
    assert network_index(2, 5) == [0, 1, 0, 0, 0]                   # SAC_agents.py:72-75, :93-96: network 0 beyond the list
    assert network_index(8, 3) == [0, 1, 2]
    assert network_index(4, 6, only_one_NN=True) == [0] * 6         # :88-92
    assert network_index(1, 3) == [0, 0, 0]
    with pytest.raises(ValueError):
        network_index(0, 3)
    fx = load("eval_n5.npz")                                        # the reference ran this very case: 2 critics, 5 agents
    assert int(fx["n_critics"]) == 2 and fx["critic_w1"].shape[0] == 2
    assert not np.array_equal(fx["V_approxs"][:, 1], fx["V_approxs_one"][:, 1])


def test_summarize_evaluation_combines_ranks():
    import torch
    n_bins, N = 4, 3
    a = torch.tensor([2.0, -10.0, -8.0, 3.0, 100.0, 1.0, 1, 0, 0, 1, 0, 0.3, 0.6, 0.9], dtype=torch.float64)
    b = torch.tensor([6.0, -30.0, -24.0, 1.0, 500.0, 5.0, 5, 1, 0, 0, 0, 0.5, 0.2, -0.9], dtype=torch.float64)
    s = summarize_evaluation(torch.stack([a, b]), n_bins)
    assert s["episodes"] == 8 and s["world_size"] == 2 and s["collision_hist"] == [6, 1, 0, 1, 0]
    assert s["mean_return"] == -5.0 and s["mean_collisions"] == 0.5 and s["mean_length"] == 75.0 and s["zero_collision_share"] == 0.75
    assert np.allclose(s["mean_advantage"], [0.1, 0.1, 0.0])
    assert summarize_evaluation(torch.stack([a, b]), n_bins, has_critic=False)["mean_advantage"] is None
