"""Host restatement of the shuffled-minibatch contract (test infrastructure; no GPU), written from the text of
include/dronesim.h, not from the kernels:

  `row_permutation`      dronesim_row_permutation: the 4-round balanced Feistel network with cycle-walking, in Python integers;
                         its round function is word 0 of the second Philox implementation of tests/sampling_ref.py
  `gather_rows`          dronesim_gather_rows for one array, as numpy indexing
  `ppo_train_minibatch`  `ppo_ref.ppo_train` with each epoch's permuted rows cut into K blocks: one critic and one actor step per
                         block in float64, the Adam step count advancing per block; the epoch's permutation is keyed by the step
                         count the critic's optimiser has reached when the epoch starts (what `PPOLearner` reads on the device)
"""
import numpy as np
import torch

from tests import learner_ref as R
from tests import ppo_ref as P
from tests.sampling_ref import philox4x32_10

M32 = 0xFFFFFFFF


def half_bits(R_):
    """h = max(1, ceil(bitlen(R - 1) / 2))."""
    return max(1, -(-int(R_ - 1).bit_length() // 2))


def feistel(v, h, seed, counter):
    """One application of the network to the Python integer v < 2^(2h)."""
    mask = (1 << h) - 1
    L, Rr = v >> h, v & mask
    for k in range(4):
        w0 = int(philox4x32_10(Rr, k, counter & M32, 0, seed & M32, (seed >> 32) & M32)[0])
        L, Rr = Rr, L ^ (w0 & mask)
    return (L << h) | Rr


def row_permutation_scalar(R_, seed, counter):
    """perm[r] for every r, one Python integer at a time (slow: small R only)."""
    h = half_bits(R_)
    out = []
    for r in range(R_):
        v = feistel(r, h, seed, counter)
        while v >= R_:
            v = feistel(v, h, seed, counter)
        out.append(v)
    return np.array(out, dtype=np.int64)


def row_permutation(R_, seed, counter):
    """The same rule with the rows walked side by side (arrays of Python-sized integers in int64: every value is below 2^32)."""
    h = half_bits(R_)
    mask = (1 << h) - 1
    k0, k1, ctr = seed & M32, (seed >> 32) & M32, counter & M32
    v = np.arange(R_, dtype=np.int64)
    todo = np.ones(R_, dtype=bool)
    while todo.any():
        x = v[todo]
        L, Rr = x >> h, x & mask
        for k in range(4):
            w0 = philox4x32_10(Rr, k, ctr, 0, k0, k1)[0].astype(np.int64)
            L, Rr = Rr, L ^ (w0 & mask)
        v[todo] = (L << h) | Rr
        todo = v >= R_
    return v


def gather_rows(src, perm, M):
    """The K = R / M blocks ``[K, M, ...]`` of ``src [R, ...]``: block b, row j = src[perm[b M + j]]."""
    R_ = len(perm)
    assert R_ % M == 0
    return src[np.asarray(perm)].reshape(R_ // M, M, *src.shape[1:])


def ppo_train_minibatch(kind, Wa, Wc, x, reward, done, act, nbr, gamma, minibatches=1, shuffle_seed=0, epochs=10, clip_eps=0.2,
                        lr_actor=1e-3, lr_critic=1e-3, max_norm=10.0, baseline="once", state=None, perms=None):
    """`ppo_ref.ppo_train` with ``minibatches = K``: per epoch the T E rows in the order of `row_permutation(T E, shuffle_seed,
    steps taken so far)` (or ``perms[epoch]`` if given), cut into K blocks of M; per block `R.grads` + `R.clip_adam` on the critic,
    then `P.actor_grads` + `R.clip_adam` on the actor, each over the block's M rows with 1 / M.  Returns `ppo_train`'s dict with
    the per-step entries as lists ``[epoch][block]`` and ``perms`` (the permutation of every epoch)."""
    T, E, N = reward.shape
    rows, K = T * E, int(minibatches)
    assert rows % K == 0
    M = rows // K
    xr = x.reshape(rows, N, -1).double()
    actr = act.reshape(rows, N, 2).double()
    G = R.returns(reward, done, gamma)
    Wa, Wc = [w.double() for w in Wa], [w.double() for w in Wc]
    zeros = lambda W: [torch.zeros_like(w) for w in W]
    if state is None:
        state = dict(cm1=zeros(Wc), cm2=zeros(Wc), am1=zeros(Wa), am2=zeros(Wa), step=0)
    logp_old = P.logp(kind, Wa, xr, actr).detach()
    V = R.forward(Wc, xr)[2][..., 0].transpose(0, 1).reshape(T, E, N)
    adv = P.advantage(G, V, nbr, baseline)
    Gr, advr = G.reshape(rows, N), adv.reshape(rows, N)
    keys = ("critic_loss", "critic_norm", "critic_grad", "actor_loss", "actor_norm", "actor")
    out = dict(G=G, Q=P.neighbour_sum(G, nbr), V=V, adv=adv, logp_old=logp_old.reshape(T, E, N), perms=[], **{k: [] for k in keys})
    cm1, cm2, am1, am2, step = state["cm1"], state["cm2"], state["am1"], state["am2"], state["step"]
    for ep in range(epochs):
        perm = row_permutation(rows, shuffle_seed, step) if perms is None else np.asarray(perms[ep], dtype=np.int64)
        assert np.array_equal(np.sort(perm), np.arange(rows))
        out["perms"].append(perm)
        for k in keys:
            out[k].append([])
        for b in range(K):
            idx = torch.as_tensor(perm[b * M:(b + 1) * M])
            step += 1
            gc, lc = R.grads(0, Wc, xr[idx], 1.0 / M, target=Gr[idx])
            Wc, cm1, cm2, nc = R.clip_adam(Wc, gc, cm1, cm2, step, lr_critic, max_norm)
            a = P.actor_grads(kind, Wa, xr[idx], actr[idx], logp_old[idx], advr[idx], clip_eps)
            Wa, am1, am2, na = R.clip_adam(Wa, a["grad"], am1, am2, step, lr_actor, max_norm)
            for k, v in zip(keys, (lc, nc, gc, a["loss"], na, a)):
                out[k][ep].append(v)
    out.update(critic_post=Wc, actor_post=Wa, state=dict(cm1=cm1, cm2=cm2, am1=am1, am2=am2, step=step))
    return out
