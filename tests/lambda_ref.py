"""Float64 torch restatement of the bootstrapped lambda-returns (TD(lambda) / GAE) and of the two learners' updates with
them: the checker of the lambda tests (test infrastructure; CPU or GPU tensors, float64).  The reference has no such
function (it trains on whole episodes, SAC_agents.py:304-307); the updates are the existing restatements' pieces
(tests/learner_ref.py, tests/ppo_ref.py) called with the new G."""
import torch

from tests import learner_ref as R
from tests import ppo_ref as P


def lambda_returns(reward, V, done, gamma, lam):
    """reward [T,E,N], V [T+1,E,N] (V[t]: the value of the observation step t acted on, V[T]: of the one after the window),
    done [T,E] or None.  Backwards from Gn = V[T]:
        G[t] = r[t]                                            where done[t]
        G[t] = r[t] + gamma ((1 - lam) V[t+1] + lam Gn)        otherwise;          A[t] = G[t] - V[t]
    Returns (G, A) float64."""
    reward, V = reward.double(), V.double()
    T = reward.shape[0]
    G = torch.zeros_like(reward)
    Gn = V[T].clone()
    for t in range(T - 1, -1, -1):
        boot = reward[t] + gamma * ((1 - lam) * V[t + 1] + lam * Gn)
        if done is not None:
            boot = torch.where(done[t].bool()[:, None], reward[t], boot)
        Gn = boot
        G[t] = Gn
    return G, G - V[:T]


def brute_force(reward, V, done, gamma, lam):
    """The definition, element by element: A[t] = sum_l (gamma lam)^l delta[t+l], stopped after the first done, with
    delta[t] = r[t] + gamma (1 - done[t]) V[t+1] - V[t]; G = A + V.  Returns (G, A) float64."""
    reward, V = reward.double(), V.double()
    T, E, N = reward.shape
    d = torch.zeros(T, E, dtype=torch.float64) if done is None else done.double()
    delta = reward + gamma * (1 - d)[:, :, None] * V[1:] - V[:T]
    A = torch.zeros_like(reward)
    for e in range(E):
        for t in range(T):
            c = 1.0
            for l in range(T - t):
                A[t, e] += c * delta[t + l, e]
                if d[t + l, e] != 0:
                    break
                c *= gamma * lam
    return A + V[:T], A


def critic_values(Wc, x):
    """V_i(x) [rows, N] float64 for rows x [rows, N, d]."""
    return R.forward([w.double() for w in Wc], x.double())[2][..., 0].transpose(0, 1)


def sa2c_train(kind, Wa, Wc, x_all, reward, done, act, nbr, gamma, lam, lr_actor=1e-3, lr_critic=1e-3, max_norm=10.0, state=None):
    """`learner_ref.sa2c_train` with bootstrapped lambda-returns: x_all [T+1,E,N,d] is the whole observation ring.
    V of the PRE-update critic over all T+1 slots -> G -> critic step -> V of the POST-update critic over x_all[:T] ->
    `learner_ref.advantage(G, V)` -> actor step."""
    T, E, N = reward.shape
    xa = x_all.reshape((T + 1) * E, N, -1).double()
    xr = xa[:T * E]
    V_all = critic_values(Wc, xa).reshape(T + 1, E, N)
    G, _ = lambda_returns(reward, V_all, done, gamma, lam)
    zeros = lambda W: [torch.zeros_like(w, dtype=torch.float64) for w in W]
    if state is None:
        state = dict(cm1=zeros(Wc), cm2=zeros(Wc), am1=zeros(Wa), am2=zeros(Wa), step=0)
    step = state["step"] + 1
    gc, lc = R.grads(0, Wc, xr, 1.0 / (T * E), target=G.reshape(T * E, N))
    mc = R.magnitude_grads(0, Wc, xr, 1.0 / (T * E), target=G.reshape(T * E, N))
    Wc2, cm1, cm2, nc = R.clip_adam(Wc, gc, state["cm1"], state["cm2"], step, lr_critic, max_norm)
    V = critic_values(Wc2, xr).reshape(T, E, N)
    w = R.advantage(G, V, nbr, done, gamma)
    kw = dict(act=act.reshape(T * E, N, 2), weight=w.reshape(T * E, N))
    ga, la = R.grads(kind, Wa, xr, 1.0 / E, **kw)
    ma = R.magnitude_grads(kind, Wa, xr, 1.0 / E, **kw)
    Wa2, am1, am2, na = R.clip_adam(Wa, ga, state["am1"], state["am2"], step, lr_actor, max_norm)
    return dict(critic_grad=gc, critic_mag=mc, critic_loss=lc, critic_norm=nc, critic_post=Wc2, actor_grad=ga, actor_mag=ma,
                actor_loss=la, actor_norm=na, actor_post=Wa2, G=G, V_all=V_all, V=V, w=w,
                state=dict(cm1=cm1, cm2=cm2, am1=am1, am2=am2, step=step))


def ppo_train(kind, Wa, Wc, x_all, reward, done, act, nbr, gamma, lam, epochs=10, clip_eps=0.2, lr_actor=1e-3, lr_critic=1e-3,
              max_norm=10.0, baseline="once", state=None):
    """`ppo_ref.ppo_train` with bootstrapped lambda-returns: the once-per-window critic forward runs over all T+1 ring
    slots x_all, G is its lambda-return, its first T slots are the V of the advantage; epochs unchanged."""
    T, E, N = reward.shape
    rows = T * E
    xa = x_all.reshape((T + 1) * E, N, -1).double()
    xr = xa[:rows]
    actr = act.reshape(rows, N, 2).double()
    Wa, Wc = [w.double() for w in Wa], [w.double() for w in Wc]
    zeros = lambda W: [torch.zeros_like(w) for w in W]
    if state is None:
        state = dict(cm1=zeros(Wc), cm2=zeros(Wc), am1=zeros(Wa), am2=zeros(Wa), step=0)
    logp_old = P.logp(kind, Wa, xr, actr).detach()
    V_all = critic_values(Wc, xa).reshape(T + 1, E, N)
    G, _ = lambda_returns(reward, V_all, done, gamma, lam)
    V = V_all[:T]
    adv = P.advantage(G, V, nbr, baseline)
    out = dict(G=G, Q=P.neighbour_sum(G, nbr), V=V, V_all=V_all, adv=adv, logp_old=logp_old.reshape(T, E, N), critic_loss=[],
               critic_norm=[], critic_grad=[], actor_loss=[], actor_norm=[], actor=[])
    cm1, cm2, am1, am2, step = state["cm1"], state["cm2"], state["am1"], state["am2"], state["step"]
    for _ in range(epochs):
        step += 1
        gc, lc = R.grads(0, Wc, xr, 1.0 / rows, target=G.reshape(rows, N))
        Wc, cm1, cm2, nc = R.clip_adam(Wc, gc, cm1, cm2, step, lr_critic, max_norm)
        a = P.actor_grads(kind, Wa, xr, actr, logp_old, adv.reshape(rows, N), clip_eps)
        Wa, am1, am2, na = R.clip_adam(Wa, a["grad"], am1, am2, step, lr_actor, max_norm)
        out["critic_loss"].append(lc); out["critic_norm"].append(nc); out["critic_grad"].append(gc)
        out["actor_loss"].append(a["loss"]); out["actor_norm"].append(na); out["actor"].append(a)
    out.update(critic_post=Wc, actor_post=Wa, state=dict(cm1=cm1, cm2=cm2, am1=am1, am2=am2, step=step))
    return out
