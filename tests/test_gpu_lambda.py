"""GPU tests of the bootstrapped lambda-returns (TD(lambda) / GAE; `dronesim_lambda_returns`, csrc/dronesim.hip) and of
the two learners' ``lam`` path, against the float64 restatement tests/lambda_ref.py."""
import numpy as np
import pytest

from tests import lambda_ref as L
from tests import learner_ref as R
from tests import test_gpu_learner as TG

pytestmark = pytest.mark.gpu
NAMES = R.NAMES
DEV = TG.DEV
STAGE = 8                                   # time steps per stage of the scan (kRetStageT)
LAMS = (0.0, 0.5, 0.95, 1.0)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


def f32(x):
    """The float32 value the kernel receives, as a Python float (the restatement gets the same parameter)."""
    return float(np.float32(x))


def kernel_bar(torch, T, ref_G, V):
    """The project's bar for its scans, rtol 2e-5 and atol 2e-5 x scale, with the worst-case linear bound of the recurrence's
    three roundings per step, 3 T 2^-24, where that is larger (beyond T ~ 110)."""
    scale = max(1.0, float(ref_G.abs().max()), float(V.abs().max()))
    return 2e-5, max(2e-5, 3 * T * 2.0 ** -24) * scale


def assert_close(torch, got, ref, rtol, atol, what):
    err = (got.double() - ref).abs()
    excess = err - (atol + rtol * ref.abs())
    print(f"{what}: max |err| {float(err.max()):.3e}, atol {atol:.3e}, worst excess {float(excess.max()):.3e}")
    assert bool(torch.isfinite(got).all()), what
    assert float(excess.max()) <= 0.0, f"{what}: {int((excess > 0).sum())} / {excess.numel()} outside, worst excess {float(excess.max()):.3e}"


# 1 --------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 3, 5), (STAGE - 1, 5, 3), (STAGE, 5, 3), (STAGE + 1, 5, 3), (2 * STAGE, 9, 5), (2 * STAGE + 1, 9, 5),
          # the per-thread done path (a wave's columns span more than 8 envs) and a ragged last wave
          (13, 37, 3), (17, 70, 2), (33, 70, 4),
          # the wave-cooperative done path
          (40, 3, 64), (19, 5, 128), (200, 6, 64),
          # four columns per thread (N % 4 == 0 and 262144 <= E N < 524288): both sides of both edges, a ragged last
          # workgroup (E = 4100), a wave whose quadruple threads span 64 envs (N = 4: per-thread done flags), one env per wave (N = 256)
          (5, 4092, 64), (17, 4096, 64), (7, 4100, 64), (3, 8188, 64), (3, 8192, 64), (11, 65536, 4), (9, 1024, 256)]


@pytest.mark.parametrize("T,E,N", SHAPES, ids=[f"T{t}E{e}N{n}" for t, e, n in SHAPES])
def test_kernel_matches_the_float64_restatement(torch, T, E, N):
    """lam in {0, 0.5, 0.95, 1}, gamma in [0.5, 1] (1 included), with and without done, G only / A only / both."""
    from scalable_collision_avoidance_rl_amd.rollout_buffer import lambda_returns
    gen = torch.Generator(device=DEV).manual_seed(T * 1000003 + E * 101 + N)
    reward = torch.randn(T, E, N, device=DEV, generator=gen) * 3
    V = torch.randn(T + 1, E, N, device=DEV, generator=gen) * 5
    done = (torch.rand(T, E, device=DEV, generator=gen) < 0.15).to(torch.uint8)
    gammas = [1.0] + [f32(0.5 + 0.5 * float(u)) for u in torch.rand(3, device=DEV, generator=gen).cpu()]
    from scalable_collision_avoidance_rl_amd import _native
    import ctypes as C
    lib = _native.lib()
    for lam, gamma in zip(LAMS, gammas):
        lam = f32(lam)
        for d in (done, None):
            ref_G, ref_A = L.lambda_returns(reward, V, d, gamma, lam)
            rtol, atol = kernel_bar(torch, T, ref_G, V)
            tag = f"T={T} E={E} N={N} lam={lam:.2f} gamma={gamma:.4f} done={d is not None}"
            G, A = lambda_returns(reward, V, gamma, lam, d, want_adv=True)
            assert_close(torch, G, ref_G, rtol, atol, tag + " G (both)")
            assert_close(torch, A, ref_A, rtol, atol, tag + " A (both)")
            G1 = lambda_returns(reward, V, gamma, lam, d)
            assert_close(torch, G1, ref_G, rtol, atol, tag + " G only")
            A1 = torch.full_like(reward, float("nan"))
            rc = lib.dronesim_lambda_returns(reward.data_ptr(), None if d is None else d.data_ptr(), V.data_ptr(), gamma, lam, None,
                                             A1.data_ptr(), T, E, N, C.c_void_p(torch.cuda.current_stream().cuda_stream))
            _native.check(rc, "dronesim_lambda_returns")
            assert_close(torch, A1, ref_A, rtol, atol, tag + " A only")


# 2 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,E,N", [(13, 37, 3), (5, 4096, 64), (3, 8192, 64)], ids=["narrow", "wide", "above_the_wide_window"])
def test_lam_one_with_done_at_the_last_step_is_bit_identical_to_mc_returns(torch, T, E, N):
    from scalable_collision_avoidance_rl_amd.rollout_buffer import lambda_returns, mc_returns
    gen = torch.Generator(device=DEV).manual_seed(T + E + N)
    reward = torch.randn(T, E, N, device=DEV, generator=gen) * 3
    V = torch.randn(T + 1, E, N, device=DEV, generator=gen) * 5
    done = (torch.rand(T, E, device=DEV, generator=gen) < 0.15).to(torch.uint8)
    done[T - 1] = 1
    G = lambda_returns(reward, V, 0.97, 1.0, done)
    assert torch.equal(G, mc_returns(reward, 0.97, done))


def test_two_runs_are_bit_identical(torch):
    from scalable_collision_avoidance_rl_amd.rollout_buffer import lambda_returns
    T, E, N = 33, 70, 4
    gen = torch.Generator(device=DEV).manual_seed(8)
    reward = torch.randn(T, E, N, device=DEV, generator=gen) * 3
    V = torch.randn(T + 1, E, N, device=DEV, generator=gen) * 5
    done = (torch.rand(T, E, device=DEV, generator=gen) < 0.15).to(torch.uint8)
    a, b = (lambda_returns(reward, V, 0.98, 0.9, done, want_adv=True) for _ in range(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[1]).all())


# 3 --------------------------------------------------------------------------------------------------------------------
N_CUT, G_CUT, E_CUT, T_CUT, GAMMA = 5, 5.0, 64, 24, 0.99


def cut_setup(torch, make_learner=None, seed_env=5):
    """A batched auto_reset env of which every second env hits the time limit inside a T = 24 window (at step index 12 ..
    19, none at the last step) and starts a new episode that the window's end cuts; a softmax-16 actor, a critic, a real
    RolloutStorage, and the learner `make_learner(actor, critic)` builds."""
    from scalable_collision_avoidance_rl_amd import drones
    from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
    from scalable_collision_avoidance_rl_amd.rollout_buffer import RolloutStorage
    N, E, T = N_CUT, E_CUT, T_CUT
    gp = torch.Generator().manual_seed(0)
    rw = lambda *s: (torch.rand(*s, generator=gp) * 2 - 1) * 0.2
    wa = [rw(N, 6, 48), rw(N, 48), rw(N, 48, 48), rw(N, 48), rw(N, 48, 16), rw(N, 16)]
    wc = [rw(N, 6, 32), rw(N, 32), rw(N, 32, 32), rw(N, 32), rw(N, 32, 1), rw(N, 1)]
    env = drones(N, 0, [G_CUT, G_CUT], "O", k_closest=2, deltas=np.ones(N), simplify_zstate=True, n_envs=E, batched=True,
                 device=DEV, seed=seed_env, auto_reset=True)
    e = torch.arange(E, device=DEV)
    env.t.copy_(torch.where(e % 2 == 0, 180 + (e // 2) % 8, torch.zeros_like(e)).to(env.t.dtype))
    actor, critic = BatchedMLP(*wa, 1, 1, device=DEV, seed=7), BatchedMLP(*wc, 0, 0, device=DEV)
    st = RolloutStorage(env, T, actions=True)
    return env, actor, critic, st, (None if make_learner is None else make_learner(actor, critic))


def weights_of(mlp):
    return [getattr(mlp, n).detach().cpu().clone() for n in NAMES]


def ring_values(critic, st):
    T, E, N = st.reward.shape
    return critic.forward(st.z_all.view((T + 1) * E, N, -1)).view(T + 1, E, N)


def test_storage_window_that_cuts_episodes(torch):
    env, actor, critic, st, _ = cut_setup(torch)
    T, E, N = T_CUT, E_CUT, N_CUT
    TG.rollout_window(env, actor, st)
    torch.cuda.synchronize()
    ends = st.done.long().sum(0)
    assert int(st.done[T - 1].sum()) == 0 and int(ends.max()) == 1 and E // 4 <= int(ends.sum()) <= 3 * E // 4, ends.tolist()
    assert st.z_all.data_ptr() == st.zbuf.data_ptr() and tuple(st.z_all.shape) == (T + 1, E, N, 6)
    assert st.nbr_all.data_ptr() == st.nbrbuf.data_ptr() and tuple(st.nbr_all.shape) == (T + 1, E, N, 3)
    assert torch.equal(st.z_all[:T], st.z_pre) and torch.equal(st.z_all[1:], st.z)
    V = ring_values(critic, st)
    gamma = f32(GAMMA)
    # against the restatement
    for lam in (f32(0.95), 1.0):
        G, A = st.lambda_returns(V, gamma, lam, want_adv=True)
        ref_G, ref_A = L.lambda_returns(st.reward, V, st.done, gamma, lam)
        rtol, atol = kernel_bar(torch, T, ref_G, V)
        assert_close(torch, G, ref_G, rtol, atol, f"storage G lam={lam}")
        assert_close(torch, A, ref_A, rtol, atol, f"storage A lam={lam}")
    Gt = st.lambda_returns(V, gamma, 1.0, true_rewards=True)
    assert_close(torch, Gt, L.lambda_returns(st.true_reward, V, st.done, gamma, 1.0)[0], rtol, atol, "storage G of the true rewards")
    # lam = 1 against the window-truncated Monte-Carlo returns: columns without an episode end differ by gamma^(T-t) V[T];
    # the others agree up to and including their done step, and differ after it in the same way
    G1, mc = st.lambda_returns(V, gamma, 1.0), st.returns(gamma)
    tail = (gamma ** torch.arange(T, 0, -1, dtype=torch.float64, device=DEV))[:, None, None] * V[T].double()
    whole = ends == 0
    assert_close(torch, (G1.double() - mc.double())[:, whole], tail[:, whole], rtol, atol, "bootstrap tail, no episode end")
    first = torch.argmax(st.done.long(), 0)                                   # (the only end of the envs that have one)
    pre = (torch.arange(T, device=DEV)[:, None] <= first[None]) & ~whole[None]
    assert bool(pre.any()) and torch.equal(G1[pre], mc[pre])
    post = ~pre & ~whole[None]
    assert_close(torch, (G1.double() - mc.double())[post], tail.expand(T, E, N)[post], rtol, atol, "bootstrap tail, after the end")
    assert float((G1 - mc)[post].abs().max()) > 0


# 4 --------------------------------------------------------------------------------------------------------------------
def test_two_sa2c_trains_with_lam_match_float64(torch):
    """Two windows that cut episodes, each followed by `SA2CLearner(lam=0.95).train`: the pre-update critic over all T+1 ring
    slots, G, the critic step, w from the post-update critic, the actor step -- against the float64 restatement chained with
    its own Adam state.  Gradients at `test_gpu_learner.assert_grads`' bar and factor."""
    from scalable_collision_avoidance_rl_amd.learner import SA2CLearner
    lam, gamma = f32(0.95), f32(GAMMA)
    env, actor, critic, st, learner = cut_setup(torch, lambda a, c: SA2CLearner(a, c, gamma, lam=lam))
    T, E, N = T_CUT, E_CUT, N_CUT
    state = None
    for window in range(2):
        TG.rollout_window(env, actor, st)
        torch.cuda.synchronize()
        Wa, Wc = weights_of(actor), weights_of(critic)
        data = [t.cpu().clone() for t in (st.z_all, st.reward, st.done, st.actions, st.nbr_pre)]
        out = learner.train(st)
        torch.cuda.synchronize()
        ref = L.sa2c_train(1, Wa, Wc, *data, gamma, lam, state=state)
        state = ref["state"]
        if window == 0:
            assert 0 < int(data[2].sum()) < E and int(data[2][T - 1].sum()) == 0
        amax = lambda t: float(t.abs().max())
        np.testing.assert_allclose(learner.V_all.view(T + 1, E, N).cpu().numpy(), ref["V_all"].numpy(), rtol=1e-5, atol=1e-5 * amax(ref["V_all"]))
        np.testing.assert_allclose(learner.G.cpu().numpy(), ref["G"].numpy(), rtol=1e-5, atol=1e-5 * amax(ref["G"]))
        np.testing.assert_allclose(learner.w.cpu().numpy(), ref["w"].numpy(), rtol=1e-4, atol=1e-5 * amax(ref["w"]))
        np.testing.assert_allclose(out["critic_loss"].cpu().numpy(), ref["critic_loss"].numpy(), rtol=1e-5)
        np.testing.assert_allclose(out["critic_grad_norm"].cpu().numpy(), ref["critic_norm"].numpy(), rtol=1e-5)
        np.testing.assert_allclose(out["actor_grad_norm"].cpu().numpy(), ref["actor_norm"].numpy(), rtol=1e-5)
        # the gradient buffers hold the clipped gradients after the Adam step: the restatement's, times its clip factor
        for what, runner, mlp, g, mag, norm in (("critic", learner._critic_grad, critic, ref["critic_grad"], ref["critic_mag"], ref["critic_norm"]),
                                                ("actor", learner._actor_grad, actor, ref["actor_grad"], ref["actor_mag"], ref["actor_norm"])):
            coef = torch.clamp(10.0 / (norm + 1e-6), max=1.0)
            c = lambda t: t * coef.view(-1, *([1] * (t.dim() - 1)))
            TG.assert_grads(TG.split(torch, runner.grad, mlp), [c(t) for t in g], [c(t) for t in mag], f"window {window} {what}")
        for opt, mlp, post, m2 in ((learner.critic_opt, critic, ref["critic_post"], ref["state"]["cm2"]),
                                   (learner.actor_opt, actor, ref["actor_post"], ref["state"]["am2"])):
            assert int(opt.steps.min()) == int(opt.steps.max()) == window + 1
            for name, p, v in zip(NAMES, post, m2):
                got = getattr(mlp, name).double().cpu()
                sharp = v.sqrt() > 1e-3 * float(v.sqrt().max())
                tol = torch.where(sharp, torch.full_like(p, 1e-6 + 1e-3 * opt.lr), torch.full_like(p, 2 * opt.lr))
                assert torch.all((got - p).abs() <= tol), (window, name, float(((got - p).abs() - tol).max()))


# 5 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam,baseline", [(0.95, "once"), (0.95, "per_neighbour"), (1.0, "once"), (1.0, "per_neighbour")])
def test_three_ppo_epochs_with_lam_match_float64(torch, lam, baseline):
    """One window that cuts episodes, then `PPOLearner(lam=..., epochs=3).train`, at the bar of
    `test_gpu_ppo.test_four_epochs_on_a_rollout_storage_match_float64`."""
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    epochs, lam, gamma = 3, f32(lam), f32(GAMMA)
    env, actor, critic, st, learner = cut_setup(torch, lambda a, c: PPOLearner(a, c, gamma, epochs=epochs, baseline=baseline, lam=lam))
    T, E, N = T_CUT, E_CUT, N_CUT
    TG.rollout_window(env, actor, st)
    torch.cuda.synchronize()
    Wa, Wc = weights_of(actor), weights_of(critic)
    data = [t.cpu().clone() for t in (st.z_all, st.reward, st.done, st.actions, st.nbr_pre)]
    assert 0 < int(data[2].sum()) < E and int(data[2][T - 1].sum()) == 0
    out = learner.train(st)
    torch.cuda.synchronize()
    ref = L.ppo_train(1, Wa, Wc, *data, gamma, lam, epochs=epochs, baseline=baseline)
    amax = lambda t: float(t.abs().max())
    assert learner.V.data_ptr() == learner.V_all.data_ptr()             # V is the first T E rows of the one widened forward
    np.testing.assert_allclose(learner.V_all.view(T + 1, E, N).cpu().numpy(), ref["V_all"].numpy(), rtol=1e-5, atol=1e-5 * amax(ref["V_all"]))
    np.testing.assert_allclose(learner.G.cpu().numpy(), ref["G"].numpy(), rtol=1e-5, atol=1e-5 * amax(ref["G"]))
    np.testing.assert_allclose(learner.adv.cpu().numpy(), ref["adv"].numpy(), rtol=1e-4, atol=1e-5 * amax(ref["adv"]))
    c = 1.0 if baseline == "once" else (data[4] >= 0).sum(-1).to(DEV)
    Q = learner.adv + c * learner.V.view(T, E, N)
    np.testing.assert_allclose(Q.cpu().numpy(), ref["Q"].numpy(), rtol=1e-4, atol=1e-5 * amax(ref["Q"]))
    rows = T * E
    for ep in range(epochs):
        a = ref["actor"][ep]
        near = a["near"].sum(0)
        count = torch.round(out["clip_fraction"][ep].double().cpu() * rows).long()
        print(lam, baseline, "epoch", ep, "clipped", count.tolist(), "ref", a["clipped"].sum(0).tolist(), "near an edge", near.tolist(),
              "r in", float(a["r"].min()), float(a["r"].max()))
        assert torch.all((count - a["clipped"].sum(0)).abs() <= near), (ep, count, a["clipped"].sum(0), near)
        np.testing.assert_allclose(out["critic_loss"][ep].cpu().numpy(), ref["critic_loss"][ep].numpy(), rtol=1e-5)
        np.testing.assert_allclose(out["critic_grad_norm"][ep].cpu().numpy(), ref["critic_norm"][ep].numpy(), rtol=1e-5)
        np.testing.assert_allclose(out["actor_grad_norm"][ep].cpu().numpy(), ref["actor_norm"][ep].numpy(), rtol=1e-5)
        aref = a["loss"].numpy()
        np.testing.assert_allclose(out["actor_loss"][ep].cpu().numpy(), aref, rtol=1e-4, atol=1e-4 * np.abs(aref).max())
    # epoch 0: the ratio is exactly 1
    zero, one = torch.zeros(N, device=DEV), torch.ones(N, device=DEV)
    assert torch.equal(out["clip_fraction"][0], zero) and torch.equal(out["approx_kl"][0], zero)
    assert torch.equal(out["ratio_min"][0], one) and torch.equal(out["ratio_max"][0], one)
    for opt, mlp, post, m2 in ((learner.critic_opt, critic, ref["critic_post"], ref["state"]["cm2"]),
                               (learner.actor_opt, actor, ref["actor_post"], ref["state"]["am2"])):
        assert int(opt.steps.min()) == int(opt.steps.max()) == epochs
        for name, p, v in zip(NAMES, post, m2):
            got = getattr(mlp, name).double().cpu()
            sharp = v.sqrt() > 1e-3 * float(v.sqrt().max())
            tol = epochs * torch.where(sharp, torch.full_like(p, 1e-6 + 1e-3 * opt.lr), torch.full_like(p, 2 * opt.lr))
            assert torch.all((got - p).abs() <= tol), (name, float(((got - p).abs() - tol).max()))


# 6 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["sa2c", "ppo"])
def test_lam_none_is_the_learner_without_the_argument_bit_for_bit(torch, which):
    """``lam=None`` is today's path: on a storage-like object WITHOUT the ring, two learners from the same weights -- one
    built with ``lam=None``, one without the argument -- leave the same bits everywhere."""
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner, SA2CLearner
    N, E, T, d_in = 6, 9, 41, 6
    gen = torch.Generator().manual_seed(17)
    Wa, Wc = TG.random_net(torch, gen, N, d_in, 72, 40, 16), TG.random_net(torch, gen, N, d_in, 40, 33, 1)
    x, _, act, _ = TG.random_rows(torch, gen, T, E, N, d_in, 16, 1)
    reward = torch.randn(T, E, N, generator=gen)
    done = torch.zeros(T, E, dtype=torch.uint8)
    done[20, ::2] = 1
    nbr = torch.stack([torch.arange(N)[None, None, :].expand(T, E, N), torch.randint(-1, N, (T, E, N), generator=gen),
                       torch.randint(0, N, (T, E, N), generator=gen)], -1).int()
    d = lambda t: t.to(DEV).contiguous()
    runs = []
    for kw in (dict(lam=None), dict()):
        actor, critic = TG.make_mlp(Wa, 1), TG.make_mlp(Wc, 0)
        learner = (SA2CLearner(actor, critic, 0.97, **kw) if which == "sa2c" else PPOLearner(actor, critic, 0.97, epochs=2, **kw))
        assert learner.lam is None
        out = learner.train(TG.storage_of(d(x), d(reward), d(done), d(act), d(nbr)))
        torch.cuda.synchronize()
        assert not hasattr(learner, "V_all")                            # no extra allocation
        extra = [learner.w] if which == "sa2c" else [learner.adv, learner.logp_old]
        runs.append([getattr(m, n).clone() for m in (actor, critic) for n in NAMES] +
                    [learner.actor_opt.m1, learner.actor_opt.m2, learner.critic_opt.m1, learner.critic_opt.m2, learner.G, learner.V] +
                    extra + [out[k].clone() for k in sorted(out)])
    for j, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), j
    assert all(torch.isfinite(t).all() for t in runs[0])


# 7 --------------------------------------------------------------------------------------------------------------------
def test_rollout_window_and_train_with_lam_in_one_graph(torch):
    """A storage window and `SA2CLearner(lam=0.95).train` captured in ONE graph: three replays equal the same sequence run
    eagerly, bit for bit (the shape of `test_gpu_learner.test_rollout_window_and_train_in_one_graph`)."""
    from scalable_collision_avoidance_rl_amd.learner import SA2CLearner
    make = lambda a, c: SA2CLearner(a, c, GAMMA, lam=0.95)
    env, actor, critic, st, learner = cut_setup(torch, make)

    def window(env, actor, st, learner):
        TG.rollout_window(env, actor, st)
        return learner.train(st)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = window(env, actor, st, learner)              # window 1 eagerly: builds the slots and the learner's buffers
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = window(env, actor, st, learner)
    env2, actor2, critic2, st2, learner2 = cut_setup(torch, make)
    snap = lambda a, c, l, s_, o: [t.clone() for t in [getattr(m, n) for m in (a, c) for n in NAMES] +
                                   [l.actor_opt.m1, l.actor_opt.m2, l.critic_opt.m1, l.critic_opt.m2, s_.z_all, l.V_all, l.G, l.w] +
                                   [o[k] for k in sorted(o)]]
    ref = []
    for _ in range(4):
        o2 = window(env2, actor2, st2, learner2)
        ref.append(snap(actor2, critic2, learner2, st2, o2))
    torch.cuda.synchronize()
    for rep in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        got = snap(actor, critic, learner, st, out)
        for j, (a, b) in enumerate(zip(got, ref[rep])):
            assert torch.equal(a, b), (rep, j)
        assert int(learner.actor_opt.steps.min()) == int(learner.critic_opt.steps.max()) == rep + 1
    assert all(torch.isfinite(t).all() for t in got)
