"""Host tier of the composed-options tests (no GPU): the option table `train_ref.ROWS` is a pairwise cover, the composed float64
restatement (tests/train_ref.py) reduces to every per-option restatement the suite already trusts, the three network-free
windows are the ones the GPU tier is written for, and the free-running float64 chain of every row keeps the margins that keep
tests/test_gpu_train_compose.py from resting on a coin flip.

Network width.  The rows train 6 -> 24 -> 16 networks, not the 6 -> 40 -> 32 of tests/test_gpu_share.py: the kink condition below
(no hidden pre-activation within n 2^-24 sum |a_i b_i| of zero, for every row of the window at every one of the W x epochs x K
steps) is a condition on about 10^7 values per PPO row, and at 40 x 32 none of the 40 seeds tried met it on the all-on row (the smallest
margin was 0.007 - 0.34 of the bound); at 24 x 16 about one seed in twenty does.

Seeds and margins.  A row's ``seed`` is the first from 0 upward at which its chain meets every condition of section 4 (the seeds
before it failed the kink condition, or -- gated rows -- left `pick_tau` no threshold with 4 bars of gap).  Measured on the CPU, per
row: the smallest kink margin over all steps (in units of the bound), per window the smallest tau gap (in bars) with the stop step
of every agent or group, and the zero-gradient share of the last step's value rows:

  p00      seed  93  kink  1.08  tau gaps 8.3 / 14.3 / 11.7 bars, stops 877 878 878  value rows clipped 0.16 / 0.02 / 0.01
  p02      seed  44  kink  1.12  tau gaps 28.2 / 14.9 / 7.2 bars, stops 687857 586857 457634
  p03      seed  25  kink  1.25  value rows clipped 0.18 / 0.21 / 0.33
  p04      seed  13  kink  1.32
  p05      seed   4  kink  2.43
  p06      seed  46  kink  1.28  tau gaps 12.0 / 8.9 / 8.2 bars, stops 5 5 5  value rows clipped 0.17 / 0.11 / 0.14
  p07      seed   7  kink  1.58  tau gaps 11.7 / 7.7 / 6.2 bars, stops 5 5 5  value rows clipped 0.16 / 0.05 / 0.05
  p08      seed   0  kink  1.03  tau gaps 18.3 / 10.2 / 7.7 bars, stops 544664 666566 466536
  p09      seed  10  kink  1.06  value rows clipped 0.23 / 0.08 / 0.20
  p10      seed  47  kink  1.17  tau gaps 21.9 / 21.0 / 8.9 bars, stops 888788 888788 868488  value rows clipped 0.08 / 0.02 / 0.03
  p11      seed   4  kink  1.11
  s0       seed   1  kink  3.80
  s2       seed   1  kink  7.30
  s3       seed   0  kink  1.15
  s4       seed   0  kink  5.98
  p_rclip  seed   6  kink  1.26  rewards clamped 0.161 / 0.018 / 0.040
  s_oclip  seed   1  kink  1.10  observations clamped 0.1476 / 0.1008 / 0.1031

The reductions of section 2 agree with the existing restatements bit for bit (largest relative difference measured: 0): the same
functions run in the same order, so no rounding bar is needed there."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import entropy_ref as EN
from tests import lambda_ref as LR
from tests import learner_ref as R
from tests import minibatch_ref as MB
from tests import obsnorm_ref as OB
from tests import ppo_guard_ref as GR
from tests import ppo_ref as P
from tests import rewnorm_ref as RW
from tests import share_ref as S
from tests import timelimit_ref as TL
from tests import train_ref as TR

N, T, E, W = TR.N, TR.T, TR.E, TR.W
ROW_IDS = [r["id"] for r in TR.ROWS]
BY_ID = {r["id"]: r for r in TR.ROWS + TR.CLAMP_ROWS}


# 1. the table ----------------------------------------------------------------------------------------------------------------
_LEGAL = {}


def constructors_accept(learner, values):
    """Whether the learners accept a full assignment of the factors, on the CPU (a normaliser there only carries statistics).  The
    checks that are functions of their own are CALLED: `_check_lam`, `_check_time_limit`, `_check_ent_coef`, `_check_minibatches`,
    `SharingMap`, `RewardNormalizer`, `_check_reward_norm`.  Two rules are written inline in the learner where no CPU call reaches
    them -- ``baseline in PPOLearner.BASELINES`` in ``__init__`` (which needs device networks) and ``T E % minibatches`` in
    ``_prepare`` (which needs a device) -- and are RESTATED below; neither excludes a level of `LEVELS` today, and a change of
    either rule has to be followed here by hand."""
    from scalable_collision_avoidance_rl_amd import learner as L
    from scalable_collision_avoidance_rl_amd.reward_norm import RewardNormalizer
    # (the cache is keyed by what these checks read; the other factors are flags no constructor check looks at)
    key = (learner,) + tuple(values.get(f) for f in ("lam", "time_limit", "ent_coef", "share", "reward_norm", "minibatches", "baseline"))
    if key not in _LEGAL:
        try:
            lam = L._check_lam(values["lam"])
            L._check_time_limit(values["time_limit"], lam)
            L._check_ent_coef(values["ent_coef"])
            share = TR._map(values["share"])
            smap = None if share is None else L.SharingMap(share, N, "cpu")
            if values["reward_norm"] is not None:
                rn = RewardNormalizer(N, TR.GAMMA, "cpu", scope=TR._map(values["reward_norm"]))
                L._check_reward_norm(rn, SimpleNamespace(n_agents=N), smap)
            if learner == "ppo":
                L._check_minibatches(values["minibatches"], 0)
                if (T * E) % values["minibatches"]:
                    raise ValueError("minibatches")
                if values["baseline"] not in L.PPOLearner.BASELINES:
                    raise ValueError("baseline")
            _LEGAL[key] = True
        except ValueError:
            _LEGAL[key] = False
    return _LEGAL[key]


def legal_pairs():
    """Every (f, a, g, b) with f a key factor that SOME full assignment the constructors accept contains; a factor only
    `PPOLearner` has is paired on its rows only.  A pair of factors that BOTH learners have is pooled over the two learners
    ("occurs in some row"): it may be covered by a row of either, although the two learners take different code paths -- per learner
    the cover would need more rows than the table may hold."""
    if _LEGAL.get("pairs") is not None:
        return _LEGAL["pairs"]
    need = _LEGAL["pairs"] = set()
    for learner, factors in TR.FACTORS.items():
        for values in itertools.product(*[TR.LEVELS[f] for f in factors]):
            row = dict(zip(factors, values))
            if not constructors_accept(learner, row):
                continue
            for f in TR.KEY_FACTORS:
                for g in factors:
                    if g != f and not (g in TR.KEY_FACTORS and g < f):
                        need.add((f, row[f], g, row[g]))
    return need


def pairs_of(rows):
    got = set()
    for row in rows:
        for f in TR.KEY_FACTORS:
            for g in TR.FACTORS[row["learner"]]:
                if g != f:
                    got.add((f, row[f], g, row[g]))
    return got


def test_rows_are_a_pairwise_cover_of_the_combinations_the_constructors_accept():
    """For every pair of factors of which one is obs_norm, reward_norm, time_limit or share, every combination of levels that
    occurs in an assignment the constructors accept occurs in a row.  A condition: no pair may be missing.  (Deleting any single
    row of ROWS leaves pairs uncovered: `test_every_row_of_the_table_is_needed`.)"""
    ppo, sa2c = [r for r in TR.ROWS if r["learner"] == "ppo"], [r for r in TR.ROWS if r["learner"] == "sa2c"]
    assert 1 <= len(ppo) <= 12 and 1 <= len(sa2c) <= 6
    for row in TR.ROWS + TR.CLAMP_ROWS:
        assert all(row[f] in TR.LEVELS[f] for f in TR.FACTORS[row["learner"]]), row["id"]
        assert constructors_accept(row["learner"], {f: row[f] for f in TR.FACTORS[row["learner"]]}), row["id"]
    for learner, name in TR.ALL_ON.items():
        row = BY_ID[name]
        assert row["learner"] == learner and all(row[f] == TR.LEVELS[f][-1] or f in ("kind", "lam") for f in TR.FACTORS[learner]), name
        assert row["lam"] == 0.95
    need = legal_pairs()
    assert ("time_limit", "bootstrap", "lam", None) not in need and ("reward_norm", "map", "share", "all") not in need
    assert ("reward_norm", "map", "share", "map") in need and len(need) > 200
    missing = sorted(need - pairs_of(TR.ROWS), key=str)
    assert not missing, f"{len(missing)} legal pairs occur in no row: {missing}"


def test_every_row_of_the_table_is_needed():
    need = legal_pairs()
    for row in TR.ROWS:
        rest = [r for r in TR.ROWS if r is not row]
        assert need - pairs_of(rest), f"row {row['id']} covers nothing the others do not"


# 2. the composed restatement reduces to the existing ones -----------------------------------------------------------------------
def first_window(kind, share=None, seed=11):
    win = TR.windows_of(kind)[0]
    Wa, Wc = TR.tied_nets(kind, share, seed)
    data = (win["z_pre"], win["reward"], win["done"], win["actions"], win["nbr_pre"])
    return win, Wa, Wc, data


def same(a, b, what):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    assert a.shape == b.shape and torch.equal(a.double(), b.double()), (what, float((a.double() - b.double()).abs().max()))


def same_lists(a, b, what):
    assert len(a) == len(b), what
    for j, (s, t) in enumerate(zip(a, b)):
        same(s, t, (what, j))


def same_update(out, ref, what, steps=None):
    """Losses, norms, the post-update weights and second moments: the same functions in the same order, so equal bits."""
    for k in ("critic_loss", "critic_norm", "actor_loss", "actor_norm"):
        if isinstance(ref[k], list):
            flat = [v for ep in ref[k] for v in (ep if isinstance(ep, list) else [ep])]
            same_lists(out[k], flat, (what, k))
        else:
            same(out[k], ref[k], (what, k))
    same(out["G"], ref["G"], (what, "G"))
    same_lists(out["critic_post"], ref["critic_post"], (what, "critic_post"))
    same_lists(out["actor_post"], ref["actor_post"], (what, "actor_post"))


@pytest.mark.parametrize("kind", [1, 2])
def test_with_no_option_it_is_learner_ref_and_ppo_ref(kind):
    win, Wa, Wc, data = first_window(kind)
    opts = TR.options(kind=kind, epochs=3)
    out, new = TR.sa2c_window(TR.fresh_state(Wa, Wc, opts), win, opts)
    ref = R.sa2c_train(kind, Wa, Wc, *data, TR.GAMMA)
    same_update(out, ref, "sa2c")
    same(out["w"], ref["w"], "w")
    same_lists(new["cm2"], ref["state"]["cm2"], "cm2")
    out, new = TR.ppo_window(TR.fresh_state(Wa, Wc, opts), win, opts)
    ref = P.ppo_train(kind, Wa, Wc, *data, TR.GAMMA, epochs=3)
    same_update(out, ref, "ppo")
    same(out["adv"], ref["adv"], "adv")
    same(out["logp_old"], ref["logp_old"], "logp_old")
    same_lists(new["am1"], ref["state"]["am1"], "am1")
    assert new["critic_steps"] == 3 and new["actor_steps"].tolist() == [3] * N


@pytest.mark.parametrize("lam", [0.95, 1.0])
def test_with_lam_alone_it_is_lambda_ref(lam):
    win, Wa, Wc, data = first_window(1)
    ring = (win["z_all"],) + data[1:]
    opts = TR.options(kind=1, lam=lam, epochs=2)
    out, _ = TR.sa2c_window(TR.fresh_state(Wa, Wc, opts), win, opts)
    ref = LR.sa2c_train(1, Wa, Wc, *ring, TR.GAMMA, lam)
    same_update(out, ref, "sa2c")
    same(out["w"], ref["w"], "w")
    out, _ = TR.ppo_window(TR.fresh_state(Wa, Wc, opts), win, opts)
    ref = LR.ppo_train(1, Wa, Wc, *ring, TR.GAMMA, lam, epochs=2)
    same_update(out, ref, "ppo")
    same(out["adv"], ref["adv"], "adv")


def test_with_the_entropy_options_alone_it_is_entropy_ref():
    win, Wa, Wc, data = first_window(2)
    opts = TR.options(kind=2, ent_coef=0.01, normalize_advantage=True, epochs=2)
    out, _ = TR.ppo_window(TR.fresh_state(Wa, Wc, opts), win, opts)
    ref = EN.ppo_train(2, Wa, Wc, *data, TR.GAMMA, epochs=2, ent_coef=0.01, normalize_advantage=True)
    same_update(out, ref, "ppo")
    same(out["adv"], ref["adv"], "adv")
    same(out["adv_mean"], ref["adv_mean"], "adv_mean")
    same(out["adv_std"], ref["adv_std"], "adv_std")
    opts = TR.options(kind=2, ent_coef=0.01)
    out, _ = TR.sa2c_window(TR.fresh_state(Wa, Wc, opts), win, opts)
    ref = EN.sa2c_train(2, Wa, Wc, *data, TR.GAMMA, ent_coef=0.01)
    same_update(out, ref, "sa2c")
    same(out["entropy"], ref["entropy"], "entropy")


def test_with_minibatches_alone_it_is_minibatch_ref():
    win, Wa, Wc, data = first_window(1)
    opts = TR.options(kind=1, minibatches=4, shuffle_seed=2 ** 40 + 3, epochs=2)
    out, new = TR.ppo_window(TR.fresh_state(Wa, Wc, opts), win, opts)
    ref = MB.ppo_train_minibatch(1, Wa, Wc, *data, TR.GAMMA, minibatches=4, shuffle_seed=2 ** 40 + 3, epochs=2)
    same_update(out, ref, "ppo")
    assert all(np.array_equal(a, b) for a, b in zip(out["perms"], ref["perms"])) and len(out["perms"]) == 2
    assert new["critic_steps"] == 8


@pytest.mark.parametrize("kind", [1, 2])
def test_with_the_guards_and_what_goes_with_them_it_is_ppo_guard_ref(kind):
    win, Wa, Wc, data = first_window(kind)
    kw = dict(epochs=2, minibatches=4, shuffle_seed=7, lr_actor=3e-3, ent_coef=0.01, normalize_advantage=True, lam=0.95, vf_clip=0.05,
              baseline="per_neighbour")
    free = GR.ppo_train(kind, Wa, Wc, None, *data[1:], TR.GAMMA, x_all=win["z_all"], **kw)
    tau = float(torch.stack(free["kl"]).flatten().sort().values[-12])      # some agents stop inside the window
    ref = GR.ppo_train(kind, Wa, Wc, None, *data[1:], TR.GAMMA, x_all=win["z_all"], target_kl=tau, **kw)
    assert 0 < int(ref["actor_steps"].min()) < 8 and len(set(ref["actor_steps"].tolist())) >= 2
    opts = TR.options(kind=kind, target_kl=tau, **kw)
    out, new = TR.ppo_window(TR.fresh_state(Wa, Wc, opts), win, opts)
    same_update(out, ref, "ppo")
    same(out["adv"], ref["adv"], "adv")
    same(out["actor_steps"], ref["actor_steps"], "actor_steps")
    same_lists(out["kl"], ref["kl"], "kl")
    same_lists(out["am2"], ref["am2"], "am2")
    for j in range(8):
        same(out["active"][j][0], ref["active"][j][0], ("computed", j))
        same(out["active"][j][1], ref["active"][j][1], ("stepped", j))
        same(out["critic"][j]["zero"], ref["critic"][j]["zero"], ("zero", j))
    assert new["actor_steps"].tolist() == ref["actor_steps"].tolist()


@pytest.mark.parametrize("share", ["all", TR.MAP], ids=["all", "map"])
def test_with_share_alone_it_is_share_ref(share):
    win, Wa, Wc, data = first_window(2, share)
    opts = TR.options(kind=2, share=share)
    out, _ = TR.sa2c_window(TR.fresh_state(Wa, Wc, opts), win, opts)
    ref = S.sa2c_train(share, 2, Wa, Wc, *data, TR.GAMMA)
    same_update(out, ref, "sa2c")
    same_lists(out["cm2"], ref["cm2"], "cm2")
    kw = dict(epochs=2, minibatches=4, shuffle_seed=5, lr_actor=3e-3)
    free = S.ppo_train(share, 2, Wa, Wc, *data, TR.GAMMA, **kw)
    tau = float(torch.stack(free["group_kl"])[5].max()) * 0.999           # the group that moved most stops at its sixth step
    ref = S.ppo_train(share, 2, Wa, Wc, *data, TR.GAMMA, target_kl=tau, **kw)
    assert int(ref["actor_steps"].min()) < 8
    opts = TR.options(kind=2, share=share, target_kl=tau, **kw)
    out, _ = TR.ppo_window(TR.fresh_state(Wa, Wc, opts), win, opts)
    same_update(out, ref, "ppo")
    same(out["actor_steps"], ref["actor_steps"], "actor_steps")
    same_lists(out["group_kl"], ref["group_kl"], "group_kl")
    same_lists(out["am2"], ref["am2"], "am2")


def test_with_time_limit_bootstrap_the_returns_are_timelimit_ref_on_the_restated_values():
    """No existing restatement of a whole update knows the bootstrap; the degenerate case is G: with ``lam`` it is
    `timelimit_ref.lambda_returns_ends` on `lambda_ref.critic_values` of the pre-update critic, and where a window has no
    time-limit end the whole update is the terminal one."""
    wins = TR.windows_of(1)
    Wa, Wc = TR.tied_nets(1, None, 11)
    boot, term = TR.options(kind=1, lam=0.95, time_limit="bootstrap"), TR.options(kind=1, lam=0.95)
    seen = set()
    for win in wins:
        a, _ = TR.sa2c_window(TR.fresh_state(Wa, Wc, boot), win, boot)
        b, _ = TR.sa2c_window(TR.fresh_state(Wa, Wc, term), win, term)
        has = bool((a["ends"] == 2).any())
        seen.add(has)
        assert torch.equal(a["G"], b["G"]) != has
        if not has:
            same_update(a, b, "no time-limit end")
        else:
            t, e = np.argwhere(a["ends"] == 2)[0]
            V = LR.critic_values(Wc, torch.from_numpy(a["z_trunc"]).reshape(E, N, -1)).reshape(1, E, N)
            want = win["reward"][t, e].double() + TR.GAMMA * V[0, e]
            same(a["G"][t, e], want, "G at the truncated end")
    assert seen == {True, False}


def test_with_obs_norm_alone_a_window_is_the_plain_update_on_observations_mapped_beforehand():
    """Two windows of `SA2CLearner(obs_norm=)` from a fresh normaliser: window 0 reads the identity map, window 1 the table of
    window 0's T E pre-step rows -- NOT of its own rows, and not of ring slot T."""
    wins = TR.windows_of(1)
    Wa, Wc = TR.tied_nets(1, None, 11)
    opts = TR.options(kind=1, obs_norm=True)
    outs, states = TR.chain("sa2c", wins[:2], Wa, Wc, opts)
    data = lambda w, x: (x, w["reward"], w["done"], w["actions"], w["nbr_pre"])
    ref0 = R.sa2c_train(1, Wa, Wc, *data(wins[0], wins[0]["z_pre"]), TR.GAMMA)
    same_update(outs[0], ref0, "window 0")
    tab = OB.table(OB.moments(wins[0]["z_pre"].reshape(T * E, -1)), 1e-8)
    x1 = OB.apply(wins[1]["z_pre"].reshape(T * E, -1), tab, 10.0).float().reshape(wins[1]["z_pre"].shape)
    ref1 = R.sa2c_train(1, ref0["actor_post"], ref0["critic_post"], *data(wins[1], x1), TR.GAMMA, state=ref0["state"])
    same_update(outs[1], ref1, "window 1")
    assert float(states[2]["obs"][0].min()) == 2 * T * E


def test_with_reward_norm_alone_a_window_is_the_plain_update_on_rewards_scaled_beforehand():
    """Two windows of `PPOLearner(reward_norm=)`: each is `ppo_ref.ppo_train` on the rewards times the scale AFTER that window has
    been merged (update first, then apply), the carry running across the boundary."""
    wins = TR.windows_of(1)
    Wa, Wc = TR.tied_nets(1, None, 11)
    opts = TR.options(kind=1, reward_norm=TR.MAP, epochs=2)
    outs, states = TR.chain("ppo", wins[:2], Wa, Wc, opts)
    group_of, G = RW.groups(TR.MAP, N)
    ret, st, ref, Wa_, Wc_ = np.zeros((E, N)), np.zeros((3, G)), None, Wa, Wc
    for w in range(2):
        win = wins[w]
        vals, ret = RW.scan(win["reward"].numpy(), win["done"].numpy(), TR.GAMMA, ret)
        st = RW.merge(st, RW.moments(vals, group_of, G))
        scale = RW.scale(st, 1e-8)[group_of]
        r = torch.from_numpy(RW.apply(win["reward"].numpy(), scale, 10.0))
        ref = P.ppo_train(1, Wa_, Wc_, win["z_pre"], r, win["done"], win["actions"], win["nbr_pre"], TR.GAMMA, epochs=2,
                          state=None if ref is None else ref["state"])
        same_update(outs[w], ref, ("window", w))
        same(outs[w]["reward_scale"], scale, "scale")
        Wa_, Wc_ = ref["actor_post"], ref["critic_post"]
    assert float(outs[0]["reward_scale"][0]) != float(outs[1]["reward_scale"][0]) != 1.0
    assert np.array_equal(states[2]["ret"], ret)


# 3. the windows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [1, 2])
def test_the_windows_are_the_ones_the_tests_are_written_for(kind):
    wins = TR.windows_of(kind)
    assert len(wins) == W
    kinds, quiet, crossing, ghost = set(), False, [], False
    for w, win in enumerate(wins):
        assert tuple(win["z_pre"].shape) == (T, E, N, TR.D_IN) and tuple(win["z_all"].shape) == (T + 1, E, N, TR.D_IN)
        assert win["z_pre"].dtype == torch.float32 and win["done"].dtype == torch.uint8 and win["nbr_pre"].dtype == torch.int32
        for k, v in win.items():
            assert bool(torch.isfinite(v.double()).all()), (w, k)
        assert torch.equal(win["z_all"][:T], win["z_pre"])
        if w + 1 < W:
            assert torch.equal(win["z_all"][T], wins[w + 1]["z_all"][0]), w
        done = win["done"].numpy()
        ends, slot_t, n_trunc, _ = TL.episode_ends(done, win["z_final"].numpy(), TR.DONE_RADIUS, 1)
        kinds |= set(np.unique(ends).tolist())
        quiet |= bool((done.sum(0) == 0).any())
        crossing.append(done[T - 1] == 0)
        ghost |= bool((win["nbr_pre"] < 0).any())
        assert bool((win["nbr_pre"][..., 0] == torch.arange(N, dtype=torch.int32)).all())        # the self entry comes first
        # every offset that decides an end stands clear of the radius
        z = win["z_final"].numpy()[done != 0]                                                    # [ends, N, d]
        dist = np.sqrt(z[..., 0].astype(np.float64) ** 2 + z[..., 1].astype(np.float64) ** 2)
        if dist.size:
            assert float(np.abs(dist - TR.DONE_RADIUS).min()) >= TR.END_MARGIN, (w, float(np.abs(dist - TR.DONE_RADIUS).min()))
        if kind == 1:
            ang = torch.atan2(win["actions"][..., 1].double(), win["actions"][..., 0].double()) * 16 / (2 * np.pi)
            assert float((ang - ang.round()).abs().max()) < 1e-6                                 # entries of the action list
    assert kinds == {0, 1, 2}, "an arrival and a time-limit end"
    assert quiet, "an env with no end in some window"
    assert bool((crossing[0] & crossing[1]).any()), "an episode across both window boundaries"
    assert ghost, "a ghost id in nbr_pre"


# 4. the free-running chain of every row -------------------------------------------------------------------------------------------
def vf_eps_of(row):
    """eps as `test_whole_window_epochs_with_the_clipped_value_loss_match_float64` takes it: a quantile (0.7, 0.5, 0.8, 0.3, 0.9, the
    first that serves) of how far the unclipped, ungated update of window 0 moves the critic's values."""
    wins, Wa, Wc = TR.row_inputs(row)
    opts = TR.row_options(dict(row, vf_clip=False, target_kl=False))
    o, _ = TR.ppo_window(TR.fresh_state(Wa, Wc, opts), wins[0], opts)
    xr = o["x"].reshape(T * E, N, -1)
    moved = (LR.critic_values(o["critic_post"], xr) - LR.critic_values(Wc, xr)).abs().flatten()
    return [float(torch.quantile(moved, q)) for q in (0.7, 0.5, 0.8, 0.3, 0.9)]


@pytest.mark.parametrize("name", ROW_IDS + [r["id"] for r in TR.CLAMP_ROWS])
def test_the_chain_of_a_row_keeps_its_margins(name):
    """At every one of the W x epochs x K steps: the kink margin above 1 (else another seed); with target_kl each window's constant
    IS `pick_tau` of that window's ungated table, with two distinct stop steps and one before the last; with vf_clip the constant
    is the quantile rule's and puts 5-50 % of the last step's rows on the zero-gradient branch in some window; no reward and no
    observation reaches a clamp -- except in the two clamp rows, where 1-20 % of the rewards / some observations do."""
    row = BY_ID[name]
    outs, states = TR.row_chain(row)
    wins = TR.windows_of(row["kind"])
    opts = TR.row_options(row)
    kink = min(o["kink"] for o in outs)
    print(name, "seed", row["seed"], "kink margin", kink)
    assert kink > 1.0, "a hidden pre-activation within the float32 forward's rounding of zero: pick another seed"
    if row["learner"] == "ppo" and row["target_kl"]:
        for w in range(W):
            table, bar = TR.ungated_table(row, states[w], wins[w], opts)
            pick = GR.pick_tau(table, bar)
            assert pick is not None, w
            tau, stops, gap = pick
            print(name, "window", w, "tau", tau, "stops", stops, "gap", gap, "bars")
            assert abs(tau - row["taus"][w]) <= 1e-9 * tau, (w, tau, row["taus"][w])
            # two distinct stop steps over the agents or groups, and a stop before the last step.  ``share="all"`` has ONE group:
            # it has one stop step per window, so of the two conditions only the second can be asked of it
            assert min(stops) < table.shape[0] and (len(set(stops)) >= 2 or table.shape[1] == 1), (w, stops)
            assert outs[w]["actor_steps"].tolist() == [stops[g] for g in S.groups_of(opts["share"], N)[0]], (w, stops)
    if row["learner"] == "ppo" and row["vf_clip"]:
        assert any(abs(row["vf_eps"] - e) <= 1e-9 * e for e in vf_eps_of(row)), (row["vf_eps"], vf_eps_of(row))
        shares = [float(o["critic"][-1]["zero"].double().mean()) for o in outs]
        print(name, "zero-gradient share of the last step per window", shares)
        assert any(0.05 <= s <= 0.5 for s in shares), shares
    if row["reward_norm"] is not None:
        clamped = [o["reward_clamped"] for o in outs]
        print(name, "rewards clamped", clamped, "largest |scaled reward| / clip", [o["reward_headroom"] for o in outs])
        if "reward_clip" in row:
            assert all(0.01 <= c <= 0.2 for c in clamped), clamped
        else:
            assert max(clamped) == 0.0, clamped
    if row["obs_norm"]:
        clamped = [o["obs_clamped"] for o in outs]
        print(name, "observations clamped", clamped, "largest |normalised| / clip", [o["obs_headroom"] for o in outs])
        if "obs_clip" in row:
            assert max(clamped) > 0.0, clamped
        else:
            assert max(clamped) == 0.0, clamped
    for o in outs:
        for k in ("G", "critic_loss", "actor_loss") if row["learner"] == "sa2c" else ("G", "adv"):
            v = o[k]
            assert bool(torch.isfinite(torch.as_tensor(v)).all()), k
