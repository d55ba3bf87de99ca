"""NumPy / float64 restatement of the two evaluation kernels' contracts (include/dronesim.h: dronesim_episode_eval,
dronesim_histogram_i32) -- test infrastructure, no GPU needed.  tests/test_evaluate_host.py checks it against plain Python
loops written from benchmark_agent.py:59-106 and against the reference's own run (tests/golden/eval_n5.npz)."""
import numpy as np


def mc_returns(reward, gamma, done=None):
    """G[t] = r[t] + gamma G[t+1], restarting where done[t] != 0 (SAC_agents.py:107-113); float64."""
    r = np.asarray(reward, np.float64)
    T = r.shape[0]
    G = np.zeros_like(r)
    for t in range(T - 1, -1, -1):
        last = np.ones(r.shape[1], bool) if t == T - 1 else (np.asarray(done[t]) != 0 if done is not None else np.zeros(r.shape[1], bool))
        nxt = G[t + 1] if t + 1 < T else np.zeros_like(r[0])
        G[t] = np.where(last[:, None], r[t], nxt * gamma + r[t])
    return G


def episode_eval(reward, true_reward, n_coll, done, V=None, gamma=0.99, G=None):
    """The first episode of every env of a window: reward, true_reward, V, G [T,E,N]; n_coll, done [T,E].
    ``G``: the returns to take for mean_adv (e.g. the kernel's own float32 ones); default: `mc_returns` in float64."""
    r = np.asarray(reward, np.float64); tr = np.asarray(true_reward, np.float64)
    T, E, N = r.shape
    done = np.asarray(done).reshape(T, E) != 0
    n_coll = np.asarray(n_coll, np.int64).reshape(T, E)
    G = mc_returns(r, gamma, done) if G is None else np.asarray(G, np.float64)
    L = np.where(done.any(0), 1 + done.argmax(0), 0).astype(np.int32) if T else np.zeros(E, np.int32)
    out = dict(ep_len=L, ep_collisions=np.zeros(E, np.int32), agent_return=np.zeros((E, N)), agent_true_return=np.zeros((E, N)),
               ep_return=np.zeros(E), ep_true_return=np.zeros(E), G=G)
    if V is not None:
        out["mean_adv"] = np.zeros((E, N))
    m = (np.arange(T)[:, None] < L[None, :]).astype(np.float64)                      # [T,E]: the steps of the first episode
    n = np.maximum(L, 1).astype(np.float64)
    out["ep_collisions"] = (n_coll * m.astype(np.int64)).sum(0).astype(np.int32)
    out["agent_return"] = (r * m[:, :, None]).sum(0)
    out["agent_true_return"] = (tr * m[:, :, None]).sum(0)
    out["ep_return"] = out["agent_return"].sum(1) / N
    out["ep_true_return"] = out["agent_true_return"].sum(1) / N
    if V is not None:
        out["mean_adv"] = ((G - np.asarray(V, np.float64)) * m[:, :, None]).sum(0) / n[:, None]
    return out


def histogram(values, n_bins, valid=None):
    """counts[min(v, n_bins)] over the entries with v >= 0 and valid != 0: int64 [n_bins + 1], the last bin is the overflow."""
    v = np.asarray(values, np.int64).reshape(-1)
    keep = v >= 0
    if valid is not None:
        keep &= np.asarray(valid).reshape(-1) != 0
    return np.bincount(np.minimum(v[keep], n_bins), minlength=n_bins + 1).astype(np.int64)


def synthetic_window(T, E, N, seed, with_V=True):
    """A seeded window with every `done` pattern the kernel has to get right, cycling over the envs: no done at all, done at
    t = 0, done only at T - 1, several dones (only the first counts), one random done."""
    rng = np.random.default_rng(seed)
    reward = (rng.standard_normal((T, E, N)) * 3 - 1).astype(np.float32)
    true_reward = (rng.standard_normal((T, E, N)) - 2).astype(np.float32)
    V = (rng.standard_normal((T, E, N)) * 5).astype(np.float32) if with_V else None
    n_coll = rng.integers(0, 4, (T, E)).astype(np.int32) * (rng.random((T, E)) < 0.3)
    done = np.zeros((T, E), np.uint8)
    for e in range(E):
        kind = (e + seed) % 5
        if kind == 1:
            done[0, e] = 1
        elif kind == 2:
            done[T - 1, e] = 1
        elif kind == 3:
            done[rng.integers(0, T, 3), e] = 1
            done[T - 1, e] = 1
        elif kind == 4:
            done[rng.integers(0, T), e] = 1
    return dict(reward=reward, true_reward=true_reward, n_coll=n_coll.astype(np.int32), done=done, V=V)
