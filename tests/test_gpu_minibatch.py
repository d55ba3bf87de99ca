"""GPU tests of the shuffled minibatches (csrc/minibatch.hip: `dronesim_row_permutation`, `dronesim_gather_rows`;
`learner.PPOLearner(minibatches=K)`) against the host restatement of the contract (tests/minibatch_ref.py) and
`torch.index_select`."""
import ctypes as C

import numpy as np
import pytest

from tests import learner_ref as R
from tests import minibatch_ref as MB
from tests import test_gpu_learner as TG
from tests import test_gpu_ppo as TP

pytestmark = pytest.mark.gpu
NAMES = R.NAMES
DEV = TG.DEV
R_LIST = (1, 2, 3, 4, 5, 63, 64, 65, 1000, 4097)
SEEDS = (12345, 2 ** 40 + 3)
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


def stream_of(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def device_permutation(torch, rows, seed, counter, out=None):
    """`dronesim_row_permutation` with the counter tensor ``counter`` (int32, device)."""
    from scalable_collision_avoidance_rl_amd import _native
    out = torch.full((rows,), -1, dtype=torch.int32, device=DEV) if out is None else out
    _native.check(_native.lib().dronesim_row_permutation(rows, seed, counter.data_ptr(), out.data_ptr(), stream_of(torch)),
                  "dronesim_row_permutation")
    return out


# 1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", R_LIST)
def test_device_permutation_equals_the_restatement(torch, rows):
    for seed in SEEDS:
        for c in (0, 1, 7):
            counter = torch.tensor([c, 99], dtype=torch.int32, device=DEV)         # (only the first entry is read)
            got = device_permutation(torch, rows, seed, counter).cpu().numpy()
            assert np.array_equal(got, MB.row_permutation(rows, seed, c)), (seed, c)


def test_bumping_the_counter_tensor_gives_the_next_permutation(torch):
    rows, seed = 1000, SEEDS[1]
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    perm = torch.empty(rows, dtype=torch.int32, device=DEV)
    first = device_permutation(torch, rows, seed, counter, perm).clone()
    counter += 1
    second = device_permutation(torch, rows, seed, counter, perm).clone()
    assert np.array_equal(first.cpu().numpy(), MB.row_permutation(rows, seed, 0))
    assert np.array_equal(second.cpu().numpy(), MB.row_permutation(rows, seed, 1))
    assert not torch.equal(first, second)


# 2 --------------------------------------------------------------------------------------------------------------------
def gather(torch, perm, M, srcs):
    """One `dronesim_gather_rows` of ``srcs`` ([R, ...] 4-byte element tensors) into sentinel-filled buffers whose blocks are
    padded to 256 bytes.  Returns, per array, (buffer as int32 words, row words, block words)."""
    from scalable_collision_avoidance_rl_amd import _native
    rows, n = perm.numel(), len(srcs)
    K = rows // M
    row_words = [int(np.prod(s.shape[1:])) for s in srcs]
    block_words = [-(-M * w * 4 // 256) * 64 for w in row_words]
    bufs = [torch.full((K * bw,), SENTINEL, dtype=torch.int32, device=DEV) for bw in block_words]
    arr = lambda ty, vals: (ty * n)(*vals)
    rc = _native.lib().dronesim_gather_rows(perm.data_ptr(), rows, M, n, arr(C.c_void_p, [s.data_ptr() for s in srcs]),
                                            arr(C.c_void_p, [b.data_ptr() for b in bufs]), arr(C.c_int64, [4 * w for w in row_words]),
                                            arr(C.c_int64, [4 * w for w in block_words]), stream_of(torch))
    _native.check(rc, "dronesim_gather_rows")
    torch.cuda.synchronize()
    return list(zip(bufs, row_words, block_words))


def check_gather(torch, perm, M, srcs, kept):
    rows = perm.numel()
    K = rows // M
    for j, ((buf, rw, bw), src, keep) in enumerate(zip(gather(torch, perm, M, srcs), srcs, kept)):
        assert torch.equal(src, keep), j                                          # the source is unchanged
        blocks = buf.view(K, bw)
        want = torch.index_select(src.view(torch.int32).reshape(rows, rw), 0, perm.long()).reshape(K, M * rw)
        assert torch.equal(blocks[:, :M * rw], want), j                           # bit for bit
        assert bool((blocks[:, M * rw:] == SENTINEL).all()), j                    # the padding was not written


def learner_arrays(torch, gen, rows, N=3, d_in=6):
    """Five arrays with the learner's row sizes at N = 3, d_in = 6 -- 72, 24, 12, 12, 12 bytes -- one of them int32."""
    f = lambda *s: torch.randn(rows, *s, generator=gen).to(DEV)
    return [f(N, d_in), f(N, 2), f(N), torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, N), generator=gen, dtype=torch.int64).int().to(DEV), f(N)]


@pytest.mark.parametrize("rows,M", [(192, 192), (192, 64), (192, 1), (4097, 241)])
def test_gather_equals_index_select_and_leaves_the_padding_alone(torch, rows, M):
    gen = torch.Generator().manual_seed(rows + M)
    srcs = learner_arrays(torch, gen, rows)
    kept = [s.clone() for s in srcs]
    perm = torch.randperm(rows, generator=gen).int().to(DEV)
    check_gather(torch, perm, M, srcs, kept)
    # the device's own permutation drives the same gather
    perm = device_permutation(torch, rows, SEEDS[0], torch.tensor([3], dtype=torch.int32, device=DEV))
    check_gather(torch, perm, M, srcs, kept)


def test_gather_of_eight_arrays_in_one_call(torch):
    """Eight arrays at once: the five above, 16- and 48-byte rows (which move as 16-byte pieces) and a 4-byte row."""
    rows, M = 192, 64
    gen = torch.Generator().manual_seed(8)
    srcs = learner_arrays(torch, gen, rows) + [torch.randn(rows, 4, generator=gen).to(DEV), torch.randn(rows, 12, generator=gen).to(DEV),
                                               torch.randn(rows, 1, generator=gen).to(DEV)]
    perm = torch.randperm(rows, generator=gen).int().to(DEV)
    check_gather(torch, perm, M, srcs, [s.clone() for s in srcs])
    # 1536-byte rows (N = 64, d_in = 6), more than one tile of positions, a ragged last tile
    rows, M = 330, 110
    srcs = [torch.randn(rows, 64, 6, generator=gen).to(DEV), torch.randn(rows, 64, generator=gen).to(DEV)]
    perm = torch.randperm(rows, generator=gen).int().to(DEV)
    check_gather(torch, perm, M, srcs, [s.clone() for s in srcs])


# 3 --------------------------------------------------------------------------------------------------------------------
def weights_of(mlp):
    return [getattr(mlp, n).detach().cpu().clone() for n in NAMES]


def compare_with_float64(torch, learner, actor, critic, out, ref, epochs, K, M, what):
    """The assertions and tolerances of tests/test_gpu_ppo.py:182-203, per minibatch; the weight tolerance scales with the
    ``epochs x K`` steps taken, the clipped-row slack is the restatement's own `near` count of the block."""
    assert np.array_equal(learner.perm.cpu().numpy(), ref["perms"][-1])
    N = actor.n_agents
    for k in ("critic_loss", "actor_loss", "critic_grad_norm", "actor_grad_norm", "clip_fraction", "approx_kl", "ratio_min", "ratio_max"):
        assert out[k].shape == (epochs, K, N), k
    for ep in range(epochs):
        for b in range(K):
            a = ref["actor"][ep][b]
            near = a["near"].sum(0)
            count = torch.round(out["clip_fraction"][ep, b].double().cpu() * M).long()
            print(what, "epoch", ep, "block", b, "clipped", count.tolist(), "ref", a["clipped"].sum(0).tolist(), "near an edge",
                  near.tolist(), "r in", float(a["r"].min()), float(a["r"].max()), "gpu r in", float(out["ratio_min"][ep, b].min()),
                  float(out["ratio_max"][ep, b].max()))
            assert torch.all((count - a["clipped"].sum(0)).abs() <= near), (ep, b, count, a["clipped"].sum(0), near)
            np.testing.assert_allclose(out["critic_loss"][ep, b].cpu().numpy(), ref["critic_loss"][ep][b].numpy(), rtol=1e-5)
            np.testing.assert_allclose(out["critic_grad_norm"][ep, b].cpu().numpy(), ref["critic_norm"][ep][b].numpy(), rtol=1e-5)
            np.testing.assert_allclose(out["actor_grad_norm"][ep, b].cpu().numpy(), ref["actor_norm"][ep][b].numpy(), rtol=1e-5)
            aref = a["loss"].numpy()
            np.testing.assert_allclose(out["actor_loss"][ep, b].cpu().numpy(), aref, rtol=1e-4, atol=1e-4 * np.abs(aref).max())
    steps = epochs * K
    for opt, mlp, post, m2 in ((learner.critic_opt, critic, ref["critic_post"], ref["state"]["cm2"]),
                               (learner.actor_opt, actor, ref["actor_post"], ref["state"]["am2"])):
        assert int(opt.steps.min()) == int(opt.steps.max()) == steps
        for name, p, v in zip(NAMES, post, m2):
            got = getattr(mlp, name).double().cpu()
            # per step taken: tight where the element's gradient scale is not tiny against its tensor's, within 2 lr elsewhere
            sharp = v.sqrt() > 1e-3 * float(v.sqrt().max())
            tol = steps * torch.where(sharp, torch.full_like(p, 1e-6 + 1e-3 * opt.lr), torch.full_like(p, 2 * opt.lr))
            print(what, name, "worst |gpu - float64|", float((got - p).abs().max()), "of tol", float(((got - p).abs() / tol).max()))
            assert torch.all((got - p).abs() <= tol), (name, float(((got - p).abs() - tol).max()))


def test_minibatch_epochs_on_a_rollout_storage_match_float64(torch):
    """The set-up of `test_gpu_ppo.storage_setup` (T E = 384 rows, N = 16, softmax-16): epochs = 2, K = 4, M = 96."""
    epochs, K, seed = 2, 4, 2 ** 40 + 3
    env, actor, critic, st, learner = TP.storage_setup(torch, epochs=epochs, minibatches=K, shuffle_seed=seed)
    T, E, N = TP.T_RS, TP.E_RS, TP.N_RS
    TG.rollout_window(env, actor, st)
    torch.cuda.synchronize()
    Wa, Wc = weights_of(actor), weights_of(critic)
    data = [t.cpu().clone() for t in (st.z_pre, st.reward, st.done, st.actions, st.nbr_pre)]
    out = learner.train(st)
    torch.cuda.synchronize()
    ref = MB.ppo_train_minibatch(1, Wa, Wc, *data, 0.99, minibatches=K, shuffle_seed=seed, epochs=epochs)
    amax = lambda t: float(t.abs().max())
    np.testing.assert_allclose(learner.G.cpu().numpy(), ref["G"].numpy(), rtol=1e-5, atol=1e-5 * amax(ref["G"]))
    np.testing.assert_allclose(learner.adv.cpu().numpy(), ref["adv"].numpy(), rtol=1e-4, atol=1e-5 * amax(ref["adv"]))
    # the gathered buffers hold the window's rows in the last epoch's order
    perm = learner.perm.long()
    for g, src in zip(learner._mb, (st.z_pre, st.actions, learner.logp_old, learner.adv, learner.G)):
        want = src.reshape(T * E, *src.shape[2:])[perm]
        assert torch.equal(torch.stack(g.blocks).reshape(want.shape), want)
        assert all(b.data_ptr() % 256 == 0 for b in g.blocks)
    compare_with_float64(torch, learner, actor, critic, out, ref, epochs, K, T * E // K, "storage")


def test_minibatch_epochs_with_a_gaussian_actor_match_float64(torch):
    """The synthetic Gaussian-actor set-up of `test_two_learners_on_the_same_data_are_bit_identical` (T E = 369 rows): K = 3."""
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    actor, critic, Wa, Wc, data = gaussian_setup(torch)
    epochs, K, seed = 3, 3, 7
    learner = PPOLearner(actor, critic, 0.97, epochs=epochs, rows_per_chunk=128, lr_actor=3e-3, minibatches=K, shuffle_seed=seed)
    d = lambda t: t.to(DEV).contiguous()
    out = learner.train(TG.storage_of(*[d(t) for t in data]))
    torch.cuda.synchronize()
    ref = MB.ppo_train_minibatch(2, Wa, Wc, *data, 0.97, minibatches=K, shuffle_seed=seed, epochs=epochs, lr_actor=3e-3)
    compare_with_float64(torch, learner, actor, critic, out, ref, epochs, K, 369 // K, "gaussian")


def gaussian_setup(torch):
    N, E, T, d_in = 6, 9, 41, 6
    gen = torch.Generator().manual_seed(17)
    Wa, Wc = TG.random_net(torch, gen, N, d_in, 72, 40, 4), TG.random_net(torch, gen, N, d_in, 40, 33, 1)
    Wa[4] = Wa[4] * R.structural_mask(2, Wa)
    x, _, act, _ = TG.random_rows(torch, gen, T, E, N, d_in, 4, 2)
    reward = torch.randn(T, E, N, generator=gen)
    done = torch.zeros(T, E, dtype=torch.uint8)
    done[20, ::2] = 1
    nbr = torch.stack([torch.arange(N)[None, None, :].expand(T, E, N), torch.randint(-1, N, (T, E, N), generator=gen),
                       torch.randint(0, N, (T, E, N), generator=gen)], -1).int()
    return TG.make_mlp(Wa, 2), TG.make_mlp(Wc, 0), Wa, Wc, (x, reward, done, act, nbr)


# 4 --------------------------------------------------------------------------------------------------------------------
def test_minibatches_compose_with_the_other_options(torch):
    """K = 4 with lam, time_limit="bootstrap", ent_coef and normalize_advantage: finite outputs of the right shapes, and step 2 is
    untouched -- G and the standardised adv equal a K = 1 learner's on the same storage and pre-update weights, bit for bit."""
    epochs, K = 2, 4
    kw = dict(epochs=epochs, lam=0.95, time_limit="bootstrap", ent_coef=0.01, normalize_advantage=True)
    res = []
    for k in (K, 1):
        env, actor, critic, st, learner = TP.storage_setup(torch, minibatches=k, **kw)
        TG.rollout_window(env, actor, st)
        out = learner.train(st)
        torch.cuda.synchronize()
        res.append((learner, out, st))
    (learner, out, st), (learner1, out1, st1) = res
    N = TP.N_RS
    assert torch.equal(st.z_pre, st1.z_pre) and torch.equal(st.done, st1.done)
    assert torch.equal(learner.G, learner1.G) and torch.equal(learner.adv, learner1.adv) and torch.equal(learner.logp_old, learner1.logp_old)
    assert torch.equal(out["adv_mean"], out1["adv_mean"]) and torch.equal(out["adv_std"], out1["adv_std"])
    assert out["adv_mean"].shape == (N,) and out["adv_std"].shape == (N,)
    for k, v in out.items():
        assert torch.isfinite(v).all(), k
        if k not in ("adv_mean", "adv_std"):
            assert v.shape == (epochs, K, N) and out1[k].shape == (epochs, N), k
    assert out["entropy"].shape == (epochs, K, N) and float(out["entropy"].min()) > 0
    assert int(learner.critic_opt.steps.min()) == int(learner.actor_opt.steps.max()) == epochs * K
    for mlp in (learner.actor, learner.critic):
        assert all(torch.isfinite(getattr(mlp, n)).all() for n in NAMES)


# 5 --------------------------------------------------------------------------------------------------------------------
def test_one_minibatch_is_the_whole_window_path(torch):
    """`PPOLearner(minibatches=1)` and `PPOLearner()`: bit-identical weights, moments and outputs; no `perm`, no gathered buffers."""
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    runs = []
    for kw in (dict(minibatches=1, shuffle_seed=99), dict()):
        actor, critic, Wa, Wc, data = gaussian_setup(torch)
        learner = PPOLearner(actor, critic, 0.97, epochs=3, rows_per_chunk=128, lr_actor=3e-3, **kw)
        out = learner.train(TG.storage_of(*[t.to(DEV).contiguous() for t in data]))
        torch.cuda.synchronize()
        assert not hasattr(learner, "perm") and not hasattr(learner, "_mb") and not hasattr(learner, "_actor_mb")
        assert all(v.shape == (3, 6) for v in out.values())
        runs.append([getattr(m, n).clone() for m in (actor, critic) for n in NAMES] +
                    [learner.actor_opt.m1, learner.actor_opt.m2, learner.critic_opt.m1, learner.critic_opt.m2, learner.adv,
                     learner.logp_old] + [out[k].clone() for k in sorted(out)])
    for j, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), j


# 6 --------------------------------------------------------------------------------------------------------------------
def snapshot(actor, critic, learner, out):
    return [t.clone() for t in [getattr(m, n) for m in (actor, critic) for n in NAMES] +
            [learner.actor_opt.m1, learner.actor_opt.m2, learner.critic_opt.m1, learner.critic_opt.m2, learner.adv, learner.logp_old,
             learner.perm] + [out[k] for k in sorted(out)]]


def test_minibatch_learners_are_deterministic_and_the_seed_matters(torch):
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    runs = []
    for seed in (5, 5, 6):
        actor, critic, Wa, Wc, data = gaussian_setup(torch)
        learner = PPOLearner(actor, critic, 0.97, epochs=3, rows_per_chunk=128, lr_actor=3e-3, minibatches=3, shuffle_seed=seed)
        out = learner.train(TG.storage_of(*[t.to(DEV).contiguous() for t in data]))
        torch.cuda.synchronize()
        runs.append(snapshot(actor, critic, learner, out))
    for j, (a, b) in enumerate(zip(runs[0], runs[1])):
        assert torch.equal(a, b), j
    assert all(torch.isfinite(t.float()).all() for t in runs[0])
    # another shuffle_seed: another permutation, other weights (actor w1, critic w1), the same once-per-window advantage
    assert not torch.equal(runs[0][18], runs[2][18])
    assert not torch.equal(runs[0][0], runs[2][0]) and not torch.equal(runs[0][6], runs[2][6])
    assert torch.equal(runs[0][16], runs[2][16]) and torch.equal(runs[0][17], runs[2][17])


def test_rollout_window_and_minibatch_train_in_one_graph(torch):
    """A storage window and `PPOLearner.train(minibatches=3)` captured in ONE graph on a side stream: two replays equal the same
    sequence run eagerly, bit for bit -- the second replay reshuffles through the device counter."""
    epochs, K = 2, 3
    kw = dict(epochs=epochs, minibatches=K, shuffle_seed=11)
    env, actor, critic, st, learner = TP.storage_setup(torch, **kw)

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
    env2, actor2, critic2, st2, learner2 = TP.storage_setup(torch, **kw)
    ref = []
    for _ in range(3):
        o2 = window(env2, actor2, st2, learner2)
        ref.append(snapshot(actor2, critic2, learner2, o2) + [st2.z_pre.clone()])
    torch.cuda.synchronize()
    perms = []
    for rep in (1, 2):
        graph.replay()
        torch.cuda.synchronize()
        got = snapshot(actor, critic, learner, out) + [st.z_pre.clone()]
        for j, (a, b) in enumerate(zip(got, ref[rep])):
            assert torch.equal(a, b), (rep, j)
        assert int(learner.actor_opt.steps.min()) == int(learner.critic_opt.steps.max()) == epochs * K * (rep + 1)
        perms.append(learner.perm.clone())
        assert np.array_equal(perms[-1].cpu().numpy(), MB.row_permutation(TP.T_RS * TP.E_RS, 11, epochs * K * (rep + 1) - K))
    assert not torch.equal(perms[0], perms[1])
    assert all(torch.isfinite(t.float()).all() for t in got)
