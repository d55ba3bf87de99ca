"""`BatchedMLP.sample_action` against the host restatement of its sampling tail (tests/sampling_ref.py), draw by draw, for every policy
kernel family.  Run with `-m gpu` on the MI355X box.

Every check reads the kernel's OWN `return_outputs` probabilities / (mu, var) and feeds them to the restatement together with the
Philox words the documented stream gives that (env row, agent): what is under test is the tail (csrc/policy_common.hpp: finish_quad --
quad scans, pick, unit vector, Box-Muller) and each family's mapping of (row, agent, quad part) to lanes and its loads of t[e] /
episode[e], not the matrix part (tests/test_gpu_parity.py).  That is also why plain bf16 is held to exactness here.

Bars: the categorical pick is EXACT on every draw further than delta = nout * 2^-23 from a cdf value (tests/sampling_ref.py: the
kernel's float32 scan order is its own); at most 1e-3 of a case's draws may sit inside that band.  Actions: H.ATOL = 1e-5, for the
Gaussian scaled by the sample's own amplification, 1e-5 * (1 + r) with r = sqrt(-2 ln u1) -- include/dronesim.h claims 1e-6 absolute
per hardware function, which propagates to 1e-6 * (3 + 2 r) to first order.

What no test here can see, because it changes no output: `valid` in finish_quad's `++below` condition.  A lane beyond nout scans a
probability of 0, so its cdf is the row's total; it could only count when u >= total, where every valid lane counts too and the clamp
to nout - 1 gives the same pick.  (A wrong carry of `base`, swapped Gaussian words, a family that ignores t[e] and a stream without
env_base are each reported by the first case they touch.)"""
import os
import types

import numpy as np
import pytest

from tests import helpers as H
from tests import sampling_ref as R

pytestmark = pytest.mark.gpu

# label -> (configuration, d_in, h2); h1 = 33.  "f32" at d_in = 15 falls back from the row-tile kernel to the fragment kernel
GRID = {c: (c, 6, 65) for c in H.POLICY_CONFIGS}
GRID["f32-d15"] = ("f32", 15, 65)
GRID["bf16-h129"] = ("bf16", 6, 129)
H1 = 33
WORST = {}                                                 # label -> {"categorical": worst |act - unit_action|, "gaussian": worst |act - ref| / (1 + r)}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


def host(t):
    return t.detach().cpu().numpy()


def policy(config, w, out_kind, sample_kind, seed):
    import torch
    from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
    return BatchedMLP(*[torch.from_numpy(np.ascontiguousarray(a)) for a in w], out_kind=out_kind, sample_kind=sample_kind,
                      seed=seed, device="cuda:0", **H.policy_kw(config))


def env_of(torch, t, episode, env_lo):
    """What `sample_action(env=)` reads of an env: int32 device tensors t / episode [E] and the global id of row 0."""
    if t is None:
        return None
    return types.SimpleNamespace(t=torch.tensor(np.asarray(t, np.int32), device="cuda:0"),
                                 episode=torch.tensor(np.asarray(episode, np.int32), device="cuda:0"), env_lo=int(env_lo))


def draw(pol, x, counter, env_base=0, env=None, **kw):
    """One `sample_action` at host counter `counter`: (act, idx, out) as numpy (out None without return_outputs)."""
    pol.counter = int(counter)
    res = pol.sample_action(x, env_base=env_base, env=env, **kw)
    return [None if r is None else host(r) for r in res] + [None] * (3 - len(res))


def first_bad(bad, tag, **arrays):
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} / {bad.size} draws differ; first at (e, agent) = {at}: " +
                             ", ".join(f"{k} = {v[at]!r}" for k, v in arrays.items()))


def match_picks(idx, p, words, tag, floor=0.999):
    """idx equals the restated pick on every draw outside the band; returns (compared mask, u)."""
    pick, amb, u = R.categorical_pick(p, words)
    ok = ~amb
    assert ok.mean() >= floor, f"{tag}: only {ok.mean():.4f} of the draws are outside the band"
    first_bad(ok & (idx != pick), tag, idx=idx, want=pick, u=u)
    return ok, u


def check_categorical(torch, pol, x, counter, env_base, tag, t=None, episode=None, cls=None, per_case_cap=True, stats=None):
    E, N, nout = x.shape[0], pol.n_agents, pol.nout
    env = env_of(torch, t, episode, env_base)
    act, idx, p = draw(pol, x, counter, env_base, env, return_outputs=True)
    assert idx.dtype == np.int32 and idx.shape == (E, N) and act.shape == (E, N, 2) and p.shape == (E, N, nout)
    assert idx.min() >= 0 and idx.max() < nout, tag
    words = R.draw_words(pol.seed, counter, env_base, E, N, t, episode)
    _, amb, _ = R.categorical_pick(p, words)
    if per_case_cap:
        assert amb.mean() <= R.CAP, f"{tag}: {int(amb.sum())} / {amb.size} draws inside the band"
    ok, u = match_picks(idx, p, words, tag, floor=0.999 if per_case_cap else 0.0)
    chosen = np.take_along_axis(p, idx[..., None].astype(np.int64), -1)[..., 0]
    first_bad(ok & ~(chosen > 0), tag + " (a pick of probability 0)", idx=idx, u=u)
    if cls == "uniform":
        first_bad(ok & (idx != np.minimum(np.floor(u * nout), nout - 1)), tag + " (uniform: floor(u nout))", idx=idx, u=u)
    err = np.abs(act.astype(np.float64) - R.unit_action(idx, nout))
    assert err.max() <= H.ATOL, f"{tag}: act is {err.max():.3e} from (cos, sin)(2 pi idx / nout)"
    # out == NULL: the same picks and actions, bit for bit
    act2, idx2, _ = draw(pol, x, counter, env_base, env)
    assert np.array_equal(idx2, idx) and np.array_equal(act2.view(np.uint32), act.view(np.uint32)), tag + " (return_outputs=False)"
    # idx_out / act_out as slices of a larger tensor: the same values, nothing written around them
    big_i = torch.full((E + 2, N), -7, dtype=torch.int32, device="cuda:0")
    big_a = torch.full((E + 2, N, 2), -7.0, device="cuda:0")
    draw(pol, x, counter, env_base, env, act_out=big_a[1:E + 1], idx_out=big_i[1:E + 1])
    bi, ba = host(big_i), host(big_a)
    assert np.array_equal(bi[1:E + 1], idx) and np.array_equal(ba[1:E + 1].view(np.uint32), act.view(np.uint32)), tag + " (idx_out / act_out)"
    assert np.all(bi[[0, -1]] == -7) and np.all(ba[[0, -1]] == -7.0), tag + " (wrote outside idx_out / act_out)"
    if stats is not None:
        stats["compared"] += int(ok.sum()); stats["ambiguous"] += int(amb.sum()); stats["zeros"] += int((p == 0).sum())
        stats["worst_cat"] = max(stats.get("worst_cat", 0.0), float(err.max()))
    return idx, p, ok


def check_gaussian(torch, pol, x, counter, env_base, tag, t=None, episode=None, stats=None):
    E, N = x.shape[0], pol.n_agents
    env = env_of(torch, t, episode, env_base)
    act, idx, out = draw(pol, x, counter, env_base, env, return_outputs=True)
    assert idx is None and act.shape == (E, N, 2) and out.shape == (E, N, 4)
    assert np.all(out[..., 2:] > 0) and np.all(np.abs(out[..., :2]) <= 1)
    words = R.draw_words(pol.seed, counter, env_base, E, N, t, episode)
    ref, r = R.gaussian_action(out[..., :2], out[..., 2:], words)
    err = np.abs(act.astype(np.float64) - ref) / (1.0 + r)
    first_bad(~(err <= H.ATOL), tag + f" (worst {np.nanmax(err):.3e} x (1 + r))", act=act, want=ref, r=r)
    act2, _, _ = draw(pol, x, counter, env_base, env)
    assert np.array_equal(act2.view(np.uint32), act.view(np.uint32)), tag + " (return_outputs=False)"
    big_a = torch.full((E + 2, N, 2), -7.0, device="cuda:0")
    draw(pol, x, counter, env_base, env, act_out=big_a[1:E + 1])
    ba = host(big_a)
    assert np.array_equal(ba[1:E + 1].view(np.uint32), act.view(np.uint32)) and np.all(ba[[0, -1]] == -7.0), tag + " (act_out)"
    if stats is not None:
        stats["gauss"] += act.size
        stats["worst_gauss"] = max(stats.get("worst_gauss", 0.0), float(err.max()))


def new_stats():
    return dict(compared=0, ambiguous=0, zeros=0, gauss=0)


# ------------------------------------------------------------------------------- a. categorical, exact, fixed grid
@pytest.mark.parametrize("cls", R.CLASSES)
@pytest.mark.parametrize("label", list(GRID))
def test_categorical_pick_is_the_restated_one(torch, label, cls):
    """nout in {1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32} x (N, E) in {(1, 1), (3, 65), (5, 130), (9, 257)} plus (64, 70) at nout = 16, h1 = 33,
    h2 = 65 (bf16 also 129), per weight class (ordinary; w3, b3 * 40: tails of probability exactly 0; w3 = b3 = 0: exactly uniform)."""
    config, d, h2 = GRID[label]
    stats = new_stats()
    for (nout, N, E) in R.grid_cases():
        c = R.softmax_case(cls, nout, N, E, d=d, h1=H1, h2=h2)
        pol = policy(config, c["w"], 1, 1, c["seed"])
        x = torch.from_numpy(c["x"]).cuda()
        check_categorical(torch, pol, x, c["counter"], c["env_base"], f"{label}: {c['tag']}", cls=cls, stats=stats)
    w = WORST.setdefault(label, {})
    w["categorical"] = max(w.get("categorical", 0.0), stats["worst_cat"])
    print(f"\nsampling accuracy: {label} {cls}: {stats['compared']} draws compared, {stats['ambiguous']} in the band, "
          f"{stats['zeros']} probabilities exactly 0, worst |act - unit_action| = {stats['worst_cat']:.3e}")
    assert stats["compared"] >= 0.999 * sum(N * E for (_, N, E) in R.grid_cases())
    if cls == "peaked":
        assert stats["zeros"] > 0                                      # (the class is there for the underflowed tails)


# ------------------------------------------------------------------------------- b. Gaussian, exact
@pytest.mark.parametrize("label", list(GRID))
def test_gaussian_sample_is_the_restated_one(torch, label):
    """out_kind 2, nout = 4, block-diagonal w3, the same (N, E) grid: |act - ref| <= 1e-5 (1 + r) with ref, r from the kernel's own
    (mu, var).  A swapped word pair, sin for cos or a missing sqrt move samples by O(0.1) to O(1)."""
    config, d, h2 = GRID[label]
    stats = new_stats()
    for (N, E) in R.SHAPES + (R.WIDE,):
        c = R.gaussian_case(N, E, d=d, h1=H1, h2=h2)
        pol = policy(config, c["w"], 2, 2, c["seed"])
        check_gaussian(torch, pol, torch.from_numpy(c["x"]).cuda(), c["counter"], c["env_base"], f"{label}: {c['tag']}", stats=stats)
    WORST.setdefault(label, {})["gaussian"] = stats["worst_gauss"]
    print(f"\nsampling accuracy: {label} gaussian: {stats['gauss']} samples, worst |act - ref| / (1 + r) = {stats['worst_gauss']:.3e}")
    assert stats["gauss"] == 2 * sum(N * E for (N, E) in R.SHAPES + (R.WIDE,))


# ------------------------------------------------------------------------------- c. keying
KN, KE, KNOUT = 3, 65, 9


def keying_case(torch, config, N=KN):
    c = R.softmax_case("ordinary", KNOUT, N, KE, h1=H1)
    return c, policy(config, c["w"], 1, 1, c["seed"]), torch.from_numpy(c["x"]).cuda()


def picks_match(pol, x, counter, tag, env_base=0, env=None, t=None, episode=None):
    _, idx, p = draw(pol, x, counter, env_base, env, return_outputs=True)
    base = env.env_lo if env is not None else env_base
    ok, _ = match_picks(idx, p, R.draw_words(pol.seed, counter, base, x.shape[0], pol.n_agents, t, episode), tag, floor=0.99)
    return idx, ok


@pytest.mark.parametrize("config", H.POLICY_CONFIGS)
def test_call_counter_keys_the_stream(torch, config):
    """`pol.counter` at 0, 1, 2^32 - 1 and 2^32 + 5 (the high word reaches the stream); every call advances it by exactly 1."""
    c, pol, x = keying_case(torch, config)
    seen = {}
    for counter in (0, 1, 5, 2 ** 32 - 1, 2 ** 32 + 5):
        seen[counter], _ = picks_match(pol, x, counter, f"{config}: counter = {counter}")
        assert pol.counter == counter + 1
    assert not np.array_equal(seen[5], seen[2 ** 32 + 5]) and not np.array_equal(seen[0], seen[1])
    pol.counter = 41
    pol.sample_action(x)
    _, idx, p = [host(r) for r in pol.sample_action(x, return_outputs=True)]
    match_picks(idx, p, R.draw_words(pol.seed, 42, 0, KE, KN), f"{config}: second of two calls from counter 41", floor=0.99)
    assert pol.counter == 43
    pol.forward(x)                                                 # (no draw, no advance)
    assert pol.counter == 43


@pytest.mark.parametrize("config", H.POLICY_CONFIGS)
def test_env_counters_key_the_stream(torch, config):
    """`env=`: a different t and episode per env (t = 0, t = 199, episodes above 1), env_lo = 100; the host counter stays."""
    c, pol, x = keying_case(torch, config)
    rng = np.random.default_rng(5)
    t = rng.integers(0, 200, KE).astype(np.int32); t[:3] = (0, 199, 1)
    ep = rng.integers(0, 6, KE).astype(np.int32); ep[:3] = (0, 5, 2)
    assert len(set(t)) > 30 and (ep > 1).sum() > 10
    env = env_of(torch, t, ep, 100)
    for counter in (7, 2 ** 32 - 1, (3 << 32) + 11):               # (2^32 - 1 + t wraps in the low word alone)
        with_env, ok = picks_match(pol, x, counter, f"{config}: env= at counter {counter}", env=env, t=t, episode=ep)
        assert pol.counter == counter
        flat, ok0 = picks_match(pol, x, counter, f"{config}: no env, env_base 100", env_base=100)
        same_key = (t == 0) & (ep == 0)                            # rows whose env counters are 0 draw what the call-counter path draws
        assert np.array_equal(with_env[same_key][ok[same_key] & ok0[same_key]], flat[same_key][ok[same_key] & ok0[same_key]])
        assert not np.array_equal(with_env[~same_key], flat[~same_key])


@pytest.mark.parametrize("config", H.POLICY_CONFIGS)
def test_rows_draw_by_their_global_id(torch, config):
    """Shard invariance: rows [a:] sampled with env_base + a are the tail of the full call, a in {1, 32, 64}; the global id wraps modulo
    2^32 inside the batch."""
    c, pol, x = keying_case(torch, config)
    for base in (0, 2 ** 32 - 40, c["env_base"]):
        full, ok = picks_match(pol, x, 9, f"{config}: env_base = {base}", env_base=base)
        for a in (1, 32, 64):
            part, okp = picks_match(pol, x[a:].contiguous(), 9, f"{config}: rows [{a}:] at env_base = {base} + {a}", env_base=base + a)
            both = ok[a:] & okp
            first_bad(both & (part != full[a:]), f"{config}: rows [{a}:] at env_base = {base} + {a} vs the full call", part=part, full=full[a:])


@pytest.mark.parametrize("config", H.POLICY_CONFIGS)
def test_agent_id_keys_the_stream(torch, config):
    """Agent i of an N = 3 policy and the same weights as agent i of an N = 9 policy pick the same index: the stream depends on the
    agent id, not on the launch."""
    c3, pol3, x3 = keying_case(torch, config)
    c9 = R.softmax_case("ordinary", KNOUT, 9, KE, h1=H1)
    w9 = [a.copy() for a in c9["w"]]
    for a9, a3 in zip(w9, c3["w"]):
        a9[:KN] = a3
    x9 = c9["x"].copy(); x9[:, :KN] = c3["x"]
    pol9 = policy(config, w9, 1, 1, c3["seed"])
    i3, ok3 = picks_match(pol3, x3, 12, f"{config}: N = 3", env_base=77)
    i9, ok9 = picks_match(pol9, torch.from_numpy(x9).cuda(), 12, f"{config}: N = 9", env_base=77)
    both = ok3 & ok9[:, :KN]
    first_bad(both & (i3 != i9[:, :KN]), f"{config}: agent i of N = 3 vs agent i of N = 9", n3=i3, n9=i9[:, :KN])


# ------------------------------------------------------------------------------- d. graph replay
def test_graph_replay_draws_the_restated_picks(torch):
    """sample_action(env.z, env=env, return_outputs=True) + env.step captured in a hipGraph, N = 5, E = 64, replayed three times: the
    picks of every replay are the restatement's at the env's t / episode of that replay (copied to the host before it) and the recorded
    probabilities; episodes end (and their counters move) inside the replays."""
    from scalable_collision_avoidance_rl_amd import drones
    N, E = 5, 64
    env = drones(N, 0, [5.0, 5.0], "O", k_closest=2, deltas=np.ones(N), simplify_zstate=True, n_envs=E, batched=True,
                 device="cuda:0", seed=2, auto_reset=True)
    t0 = np.random.default_rng(3).integers(0, 196, E).astype(np.int32); t0[:4] = (0, 199, 198, 197)
    env.set_state(env.pos.clone(), env.vel.clone(), t0)
    c = R.softmax_case("ordinary", 16, N, E, d=6, h1=H1)
    pol = policy("f32", c["w"], 1, 1, c["seed"])
    pol.counter = 3
    ep0 = host(env.episode).copy()

    def body():
        act, idx, out = pol.sample_action(env.z, env=env, return_outputs=True)
        env.step(act)
        return idx, out
    body(); torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        idx, out = body()
    seen = []
    for k in range(3):
        t, ep = host(env.t).copy(), host(env.episode).copy()
        graph.replay(); torch.cuda.synchronize()
        match_picks(host(idx), host(out), R.draw_words(pol.seed, 3, env.env_lo, E, N, t, ep), f"replay {k}", floor=0.99)
        seen.append(host(idx).copy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    assert pol.counter == 3
    assert int(env.t[0]) == 4                                      # 1 eager step + 3 replays (capture does not execute)
    assert list((host(env.episode) - ep0)[:4]) == [0, 1, 1, 1] and list(host(env.t)[1:4]) == [3, 2, 1]     # episodes ended at t = 199


# ------------------------------------------------------------------------------- e. seeded fuzz
@pytest.mark.parametrize("config", H.POLICY_CONFIGS)
def test_sampling_shape_fuzz(torch, config):
    """Seeded random shapes (d_in 1..16, the hidden widths of the policy shape fuzz, softmax of nout 1..32 or the Gaussian, 1..6 agents, ragged
    E incl. 1, w3 at 1x / 8x / 40x, random counter and env_base, every other iteration keyed by a per-env t / episode) with the exactness
    assertions of the fixed grid.  A single small case cannot absorb one draw inside the band, so the 1e-3 cap is asserted on the
    run's total here.  Every configuration runs the same shapes (one test per configuration)."""
    rng = np.random.default_rng(int(os.environ.get("FUZZ_SEED", 11)))
    iters = int(os.environ.get("FUZZ_ITERS", 24))
    stats, classes, kinds, softmaxes = new_stats(), set(), set(), 0
    for it in range(iters):
        d = int(rng.integers(1, 17)); N = int(rng.integers(1, 7)); E = int(rng.choice([1, 2, 31, 63, 64, 65, 130, 257]))
        h1 = int(rng.choice([1, 5, 31, 32, 33, 64, 96, 100, 128, 200, 257, 400, 512]))
        h2 = int(rng.choice([1, 7, 32, 33, 64, 65, 96, 127, 128, 129, 200, 232, 300, 400, 416, 480, 512]))
        gaussian = bool(rng.integers(0, 2)) if it >= 2 else bool(it)           # (both kinds in the shortest run)
        nout = 4 if gaussian else int(rng.integers(1, 33))
        if not gaussian and softmaxes < 4:                                     # (every nout mod 4 in the shortest run: 1, 2, 3, 0)
            nout = (nout - 1) // 4 * 4 + softmaxes + 1
        softmaxes += not gaussian
        sc3 = float(rng.choice([1.2, 9.6, 48.0]))
        w = R._network(rng, N, d, h1, h2, nout, sc3=sc3)
        if gaussian and h2 >= 2:
            w[4][:, :h2 // 2, 2:] = 0.0; w[4][:, h2 // 2:, :2] = 0.0
        x = torch.from_numpy(rng.uniform(-3.0, 3.0, (E, N, d)).astype(np.float32)).cuda()
        seed, counter, env_base = (int(rng.integers(0, 2 ** 63)) for _ in range(3))
        env_base >>= int(rng.integers(1, 40))
        t = ep = None
        if it % 2:
            t, ep = rng.integers(0, 200, E).astype(np.int32), rng.integers(0, 1000, E).astype(np.int32)
        tag = f"{config}: sampling fuzz#{it} d={d} h1={h1} h2={h2} nout={nout} gaussian={gaussian} N={N} E={E} sc3={sc3} env={t is not None}"
        pol = policy(config, w, 2 if gaussian else 1, 2 if gaussian else 1, seed)
        if gaussian:
            check_gaussian(torch, pol, x, counter, env_base, tag, t, ep, stats=stats)
        else:
            check_categorical(torch, pol, x, counter, env_base, tag, t, ep, per_case_cap=False, stats=stats)
            classes.add(nout % 4)
        kinds.add(gaussian)
    total = stats["compared"] + stats["ambiguous"]
    print(f"\nsampling fuzz {config}: {stats['compared']} categorical draws compared, {stats['ambiguous']} in the band, "
          f"{stats['gauss']} Gaussian samples, nout mod 4 seen {sorted(classes)}, "
          f"worst |act - unit_action| = {stats.get('worst_cat', 0.0):.3e}, worst Gaussian = {stats.get('worst_gauss', 0.0):.3e} x (1 + r)")
    assert kinds == {False, True}
    assert stats["ambiguous"] <= R.CAP * total and stats["gauss"] > 0 and stats["compared"] > 0
    if iters >= 24:
        assert classes == {0, 1, 2, 3} and stats["compared"] >= 1000
