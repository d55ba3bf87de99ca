"""Host side of the policy / learner seam tests (no GPU): the conditions on the INPUTS that tests/test_gpu_policy_learner_seam.py
rests on, shown with the float64 restatements alone, and the bookkeeping of the packed weight images.

  the update is large enough   one ``train()`` of every learner path moves every agent's float64 forward by at least 10 x the 1e-5
                               bar: a stale image cannot hide inside the bar
  the Gaussian share           the Gaussian networks keep (mu, var) inside the compared region on >= 99 % of the rows
  checker agreement            the two float64 `action_index` agree with j on the ideal float32 unit vectors, with margin
  image bookkeeping            `_pack()` of every mode returns the names the constructor keeps, at shapes that do not move"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import learner_ref as R
from tests import minibatch_ref as MB
from tests import ppo_guard_ref as PG
from tests import ppo_ref as P
from tests import seam_ref as S
from tests import test_gpu_learner as TG

E_HOST = min(S.envs_of(c) for c in H.POLICY_CONFIGS)          # the fewest rows any configuration trains on


def one_train(path, kind, Wa, Wc, window):
    """The float64 restatement of one ``train()`` of the learner path ``path`` (a key of `seam_ref.LEARNERS`) from fresh optimisers:
    ``(actor_post, critic_post, actor_steps or None)``."""
    k = S.OUT_KIND[kind]
    cls, kw = S.LEARNERS[path]
    if cls == "SA2CLearner":
        ref = R.sa2c_train(k, Wa, Wc, *window, S.GAMMA, lr_actor=S.LR, lr_critic=S.LR)
    elif "target_kl" in kw:
        ref = PG.ppo_train(k, Wa, Wc, *window, S.GAMMA, lr_actor=S.LR, lr_critic=S.LR, **kw)
    elif "minibatches" in kw:
        ref = MB.ppo_train_minibatch(k, Wa, Wc, *window, S.GAMMA, lr_actor=S.LR, lr_critic=S.LR, **kw)
    else:
        ref = P.ppo_train(k, Wa, Wc, *window, S.GAMMA, lr_actor=S.LR, lr_critic=S.LR, **kw)
    return ref["actor_post"], ref["critic_post"], ref.get("actor_steps")


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("path", list(S.LEARNERS))
def test_one_train_moves_every_forward_by_ten_bars(path, kind):
    """What the GPU test's teeth rest on: with the GPU tests' networks (`test_gpu_learner.storage_weights` at N = 5, 48 / 40 hidden
    units, weights uniform in +-0.2), shape (T = 6, the smallest E) and rates (1e-3, the learners' defaults), one ``train()`` moves the
    float64 forward of EVERY agent of the actor and of the critic, on the probe rows (the window's first slot), by at least 10 x the bar
    of the float32-accurate kernels.  Adam's first step moves every weight with a gradient by lr, whatever the gradient's size, so this
    does not hinge on the rewards; the frozen-actor path takes exactly one actor step."""
    Wa, Wc = TG.storage_weights(torch, S.N, S.HIDDEN, S.HIDDEN, kind)
    window = S.synthetic_window(kind, E_HOST)
    Wa2, Wc2, steps = one_train(path, kind, Wa, Wc, window)
    if path == "ppo-frozen":
        assert steps.tolist() == [1] * S.N
    if path == "ppo-guards":
        assert steps.tolist() == [3] * S.N
    probe = window[0][0]
    for what, net, before, after in (("actor", kind, Wa, Wa2), ("critic", "critic", Wc, Wc2)):
        moved = S.misses(S.forward64(after, probe, net), S.forward64(before, probe, net), "f32")
        print(path, kind, what, "moved by", [f"{v:.0f}" for v in moved.tolist()], "bars")
        assert torch.all(moved >= S.TEETH), (what, moved)


@pytest.mark.parametrize("obs_scale", [3.0, 10.0 * math.sqrt(2.0)])
def test_gaussian_networks_stay_inside_the_compared_region(obs_scale):
    """The on-policy test compares the Gaussian rows whose float64 (mu, var) have every variance in [0.05, 0.95] and every |mean| <= 0.98,
    and asks for 99 % of the rows.  With weights in +-0.2 and 20 hidden units per head the pre-activation outputs stay well inside
    +-2.9 (sigmoid) and +-2.3 (tanh): shown here for observations as large as the diagonal of the GPU tests' 10 x 10 box, before and after
    one ``train()`` of either learner."""
    Wa, Wc = TG.storage_weights(torch, S.N, S.HIDDEN, S.HIDDEN, "gaussian")
    window = S.synthetic_window("gaussian", E_HOST, obs_scale=obs_scale)
    rows = window[0].reshape(-1, S.N, S.D_IN)
    nets = [Wa] + [one_train(path, "gaussian", Wa, Wc, window)[0] for path in ("sa2c", "ppo-e3")]
    for W in nets:
        share = float(S.gaussian_region(S.forward64(W, rows, "gaussian")).double().mean())
        print("obs scale", obs_scale, "share inside", share)
        assert share >= 0.99


@pytest.mark.parametrize("nout", range(1, 33))
def test_action_index_checkers_agree_on_the_unit_vectors_with_margin(nout):
    """`learner.action_index` and `learner_ref.action_index` give j on the ideal float32 unit vectors (cos, sin)(2 pi j / nout), and
    still do with every component moved by up to +-4 float32 ulp (all 81 combinations): the nearest other entry is 2 pi / 32 = 0.196
    rad away, an ulp of a component moves the angle by about 1e-7."""
    from scalable_collision_avoidance_rl_amd.learner import action_index
    v = S.unit_vectors32(nout)                                           # [nout, 2]
    k = np.stack(np.meshgrid(np.arange(-4, 5), np.arange(-4, 5), indexing="ij"), -1).reshape(-1, 1, 2)   # [81, 1, 2]
    moved = S.step_ulps(np.broadcast_to(v, (81, nout, 2)), np.broadcast_to(k, (81, nout, 2)))
    assert np.array_equal(moved[40], v) and (moved[0] != v).all()
    want = torch.arange(nout).expand(81, nout)
    for f in (action_index, R.action_index):
        assert torch.equal(f(torch.from_numpy(moved), nout), want), f.__module__


PACK_SHAPES = [(3, 6, 48, 40, 16), (2, 6, 48, 40, 4), (2, 6, 48, 40, 1), (1, 1, 1, 1, 1), (2, 16, 33, 65, 5)]


def bare_mlp(config, w):
    """A `BatchedMLP` with only what `_pack` reads, on CPU tensors: the constructor needs the device (it raises without one), the
    packing functions are plain torch and do not."""
    from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
    kw = H.policy_kw(config)
    precision, pack_w2, split = kw.get("precision", "f32"), kw.get("pack_w2", True), kw.get("split_kernel", False)
    mlp = BatchedMLP.__new__(BatchedMLP)
    mlp.w1, mlp.b1, mlp.w2, mlp.b2, mlp.w3, mlp.b3 = w
    mlp.n_agents, mlp.d_in, mlp.h1 = w[0].shape
    mlp.h2, mlp.nout = w[4].shape[1], w[4].shape[2]
    # the constructor's mode rule (policies.py: BatchedMLP.__init__)
    if precision == "f32":
        mlp._mode = "f32" if not pack_w2 else "f32_rowtile" if pack_w2 != "fragments" and mlp.d_in <= 14 else "f32_fragments"
    elif precision == "f16x2":
        mlp._mode = "f16x2_split" if split else "f16x2_rowtile"
    else:
        mlp._mode = precision
    return mlp


@pytest.mark.parametrize("config", H.POLICY_CONFIGS)
def test_pack_returns_the_same_names_and_shapes_after_a_weight_change(config):
    """`_pack()` is what the constructor stores in `_packed` and what `refresh_weights()` copies into it, name by name: the names of a
    mode are fixed (none for the plain array of the C ABI), and shapes and types do not depend on the weights' VALUES -- zero weights,
    an in-place update and, for f16x2, other power-of-two factors included -- or `copy_` into the kept buffers would fail or broadcast.
    Every mode packs on CPU tensors, so none is skipped: the three whose stream length comes from the built library (bf16x3 and both
    f16x2: `dronesim_mlp_bf16x3_stages`, `dronesim_mlp_rt16_blocks`) ask the library, which needs no device for that."""
    from scalable_collision_avoidance_rl_amd import _native
    names = {"f32": {"w2p"}, "f32-fragments": {"w2p"}, "f32-w2-unpacked": set(), "bf16x3": {"w1p"}, "f16x2": {"wscale", "w1p"},
             "f16x2-split": {"wscale", "w1p"}, "bf16": {"w1p", "w2p", "w3p"}}[config]
    g = torch.Generator().manual_seed(5)
    for (n, d, h1, h2, nout) in PACK_SHAPES:
        if config == "f32" and d > 14:
            continue                                                    # (the row-tile stream's cap; wider inputs take the fragments)
        w = [(torch.rand(*s, generator=g) * 2 - 1) * 0.2 for s in ((n, d, h1), (n, h1), (n, h1, h2), (n, h2), (n, h2, nout), (n, nout))]
        mlp = bare_mlp(config, w)
        if config in ("bf16x3", "f16x2", "f16x2-split"):
            lib = _native.lib()
            mlp._stages = (int(lib.dronesim_mlp_rt16_blocks(h1, h2, nout)) if config == "f16x2" else int(lib.dronesim_mlp_bf16x3_stages(h1, h2)))
        first = mlp._pack()
        assert set(first) == names, (config, set(first))
        for t in w:
            t.mul_(-37.5).add_(0.01)                                     # an in-place update: other magnitudes, other f16 factors
        second = mlp._pack()
        w[0].zero_(); w[2].zero_(); w[4].zero_()
        third = mlp._pack()
        for other in (second, third):
            assert set(other) == names
            for name in names:
                assert other[name].shape == first[name].shape and other[name].dtype == first[name].dtype, (config, name)
                assert other[name].is_contiguous() and torch.isfinite(other[name].float()).all()
        assert all(not torch.equal(second[name], first[name]) for name in names)
