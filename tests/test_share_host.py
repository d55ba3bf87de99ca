"""Host-side tests of parameter sharing across agent groups: `learner.agent_groups`, the float64 restatement
(tests/share_ref.py) against ONE torch module trained on the pooled rows, and the new entry points' declarations and argument
validation (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest
import torch

from scalable_collision_avoidance_rl_amd import _native
from scalable_collision_avoidance_rl_amd.evaluate import network_index
from scalable_collision_avoidance_rl_amd.learner import agent_groups
from tests import learner_ref as R
from tests import share_ref as S
from tests import test_gpu_learner as TG
from tests import test_ppo_host as PH

NAMES = R.NAMES


# the map --------------------------------------------------------------------------------------------------------------
def test_agent_groups_all_none_and_a_non_contiguous_map():
    assert agent_groups("all", 4) == ([0, 0, 0, 0], [0, 4], [0, 1, 2, 3])
    assert agent_groups(None, 3) == ([0, 1, 2], [0, 1, 2, 3], [0, 1, 2])
    assert agent_groups([0, 1, 0, 2, 1, 0], 6) == ([0, 1, 0, 2, 1, 0], [0, 3, 5, 6], [0, 2, 5, 1, 4, 3])
    # ids are labels: any non-negative integers, numbered by the order of the groups' leaders
    assert agent_groups([7, 3, 7, 900, 3, 7], 6) == agent_groups([0, 1, 0, 2, 1, 0], 6)
    assert agent_groups((5, 5, 2), 3) == ([0, 0, 1], [0, 2, 3], [0, 1, 2])
    assert agent_groups(np.array([1, 0, 1]), 3) == ([0, 1, 0], [0, 2, 3], [0, 2, 1])
    assert agent_groups(network_index(5, 8), 8) == ([0, 1, 2, 3, 4, 0, 0, 0], [0, 4, 5, 6, 7, 8], [0, 5, 6, 7, 1, 2, 3, 4])
    assert agent_groups(network_index(1, 64), 64) == agent_groups("all", 64)


@pytest.mark.parametrize("share", ["all", None, [0, 1, 0, 2, 1, 0], [4, 4, 9, 0, 9, 4], network_index(5, 8), [3, 2, 1, 0]])
def test_agent_groups_leader_and_ordering_rules(share):
    n = 6 if share in ("all", None) else len(share)
    group_of, ptr, members = agent_groups(share, n)
    n_groups = len(ptr) - 1
    assert ptr[0] == 0 and ptr[-1] == n and sorted(members) == list(range(n)) and len(group_of) == n
    groups = [members[ptr[g]:ptr[g + 1]] for g in range(n_groups)]
    assert all(g == sorted(g) and len(g) >= 1 for g in groups)                    # ascending: the leader comes first
    leaders = [g[0] for g in groups]
    assert leaders == sorted(leaders)                                             # groups ordered by leader
    assert all(group_of[i] == k for k, g in enumerate(groups) for i in g)
    assert (group_of, groups) == S.groups_of(share, n)                            # the restatement's own reading of the rules
    ids = [0] * n if share == "all" else list(range(n)) if share is None else share
    assert all((ids[i] == ids[j]) == (group_of[i] == group_of[j]) for i in range(n) for j in range(n))


@pytest.mark.parametrize("bad", ["each", "ALL", [0, 1], [0, 1, 2, 3], [0, -1, 0], [0, 1.0, 0], [0, 0.5, 1], [0, True, 1], [False, 0, 0],
                                 [0, "1", 0], [0, None, 0], 3, 2.5, [[0], [1], [2]]])
def test_agent_groups_rejects(bad):
    with pytest.raises(ValueError):
        agent_groups(bad, 3)


# the restatement against torch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nout", [4, 1])
def test_restated_shared_update_is_one_torch_module_on_the_pooled_rows(nout):
    """Three tied agents, each with its own rows: the mean of the per-agent gradients, then `learner_ref.clip_adam` once for the
    group, against ONE torch.nn module (6 -> 8 -> 8 -> nout) trained on the pooled rows with clip_grad_norm_ and
    torch.optim.Adam in float64, over three steps.  Identical formulas at double precision: 1e-12 of each tensor's scale."""
    N, rows, d_in, h, kind, lr, max_norm = 3, 40, 6, 8, (0 if nout == 1 else 1), 3e-3, 0.05
    gen = torch.Generator().manual_seed(11 + nout)
    W = [w[[0] * N].double() for w in TG.random_net(torch, gen, N, d_in, h, h, nout)]
    x, target, act, weight = (t.reshape(rows, N, *t.shape[3:]).double() for t in TG.random_rows(torch, gen, rows, 1, N, d_in, nout, kind))
    kw = dict(target=target) if kind == 0 else dict(act=act, weight=weight)
    group_of, groups = S.groups_of("all", N)
    lin = [torch.nn.Linear(a, b).double() for a, b in ((d_in, h), (h, h), (h, nout))]
    with torch.no_grad():
        for j, layer in enumerate(lin):
            layer.weight.copy_(W[2 * j][0].T)
            layer.bias.copy_(W[2 * j + 1][0])
    net = torch.nn.Sequential(lin[0], torch.nn.ReLU(), lin[1], torch.nn.ReLU(), lin[2])
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    m1, m2 = S.zeros(W, groups), S.zeros(W, groups)
    clipped = 0
    for step in (1, 2, 3):
        g, _ = R.grads(kind, W, x, 1.0 / rows, **kw)
        W, m1, m2, norm = S.clip_adam(group_of, groups, W, g, m1, m2, step, lr, max_norm)
        # the pooled rows: one network sees every agent's rows, row scale 1 / (|G| rows)
        O = net(x.transpose(0, 1).reshape(N * rows, d_in)).reshape(N, rows, nout)
        loss = R.row_losses(kind, O, **kw).sum() / (N * rows)
        opt.zero_grad()
        loss.backward()
        tnorm = float(torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm))
        opt.step()
        clipped += tnorm > max_norm
        assert torch.all((norm - tnorm).abs() <= 1e-12 * tnorm), (step, norm, tnorm)
        for j, layer in enumerate(lin):
            for got, want in ((W[2 * j], layer.weight.detach().T), (W[2 * j + 1], layer.bias.detach())):
                assert all(torch.equal(got[0], got[i]) for i in range(N))
                assert torch.all((got[0] - want).abs() <= 1e-12 * want.abs().max()), (step, j, float((got[0] - want).abs().max()))
    assert clipped >= 1                                                           # (the clip was exercised)


def test_restated_group_mean_prescription():
    """float64 partial sums in ascending member order from the first member's value, one rounding: exact for a singleton, and
    not what a float32 running sum gives."""
    gen = torch.Generator().manual_seed(2)
    g = torch.randn(6, 5, 7, generator=gen) * torch.tensor([1e-3, 1.0, 1e3, 1.0, 1e-3, 1e3]).view(6, 1, 1)
    _, groups = S.groups_of([0, 1, 0, 2, 1, 0], 6)
    mean = S.group_mean_f32(g, groups)
    assert mean.dtype == torch.float32 and mean.shape == (3, 5, 7)
    assert torch.equal(mean[2], g[3])
    want = ((g[0].double() + g[2].double()) + g[5].double()) / 3.0
    assert torch.equal(mean[0], want.float())
    assert torch.all((mean.double() - S.group_mean(g, groups)).abs() <= 2.0 ** -24 * S.group_mean(g, groups).abs() + 1e-45)


# the C ABI ------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("dronesim_adam_step_shared", "dronesim_kl_gate_shared", "dronesim_mlp_tie")
ADAM_OK = dict(grad=4096, m1=4096, m2=4096, step=4096, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, max_norm=10.0, norm=4096, active=None,
               group_ptr=4096, members=4096, n_groups=2)
GATE_OK = dict(kl=4096, tau=0.02, active=4096, taken=4096, N=5, reset=0, group_ptr=4096, members=4096, n_groups=2)
TIE_OK = dict(group_ptr=4096, members=4096, n_groups=2)


def test_library_exports_the_sharing_entry_points_with_the_declared_argtypes():
    lib = _native.lib()
    want = ("dronesim_adam_step_shared", "dronesim_kl_gate_shared", "dronesim_mlp_tie")
    assert set(want) == set(NEW_SYMBOLS)
    header = open(_native.HEADER_PATH).read()
    for name in want:
        assert name in _native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int, name
        assert f"int {name}(" in header, name
    assert lib.dronesim_version() == 600


def test_sharing_entry_points_reject_bad_arguments_without_a_device():
    """Every EINVAL case is decided on the host, before anything is enqueued (the pointers are never dereferenced)."""
    lib = _native.lib()
    m = C.byref(PH.actor_struct())                                                # N = 5
    N = PH.actor_struct().N
    adam = lambda **kw: lib.dronesim_adam_step_shared(m, *{**ADAM_OK, **kw}.values(), None)
    for bad in (dict(grad=None), dict(m1=None), dict(m2=None), dict(step=None), dict(norm=None), dict(group_ptr=None),
                dict(members=None), dict(n_groups=0), dict(n_groups=N + 1), dict(n_groups=-1), dict(lr=-1.0), dict(b1=1.0),
                dict(eps=0.0), dict(max_norm=0.0), dict(active=4096, n_groups=0)):
        assert adam(**bad) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(b"dronesim_adam_step_shared"), bad
    assert lib.dronesim_adam_step_shared(None, *ADAM_OK.values(), None) == _native.EINVAL

    gate = lambda **kw: lib.dronesim_kl_gate_shared(*{**GATE_OK, **kw}.values(), None)
    for bad in (dict(kl=None), dict(active=None), dict(taken=None), dict(N=0), dict(tau=0.0), dict(tau=float("nan")),
                dict(tau=float("inf")), dict(group_ptr=None), dict(members=None), dict(n_groups=0), dict(n_groups=N + 1),
                dict(reset=1, group_ptr=None), dict(reset=1, n_groups=0), dict(reset=1, n_groups=N + 1), dict(reset=1, active=None)):
        assert gate(**bad) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(b"dronesim_kl_gate_shared"), bad

    tie = lambda **kw: lib.dronesim_mlp_tie(m, *{**TIE_OK, **kw}.values(), None)
    for bad in (dict(group_ptr=None), dict(members=None), dict(n_groups=0), dict(n_groups=N + 1)):
        assert tie(**bad) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(b"dronesim_mlp_tie"), bad
    assert lib.dronesim_mlp_tie(None, *TIE_OK.values(), None) == _native.EINVAL


def test_learners_and_optimiser_take_share_and_default_to_none():
    import inspect

    from scalable_collision_avoidance_rl_amd import learner as L
    from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
    for cls in (L.BatchedAdam, L.SA2CLearner, L.PPOLearner):
        assert inspect.signature(cls.__init__).parameters["share"].default is None, cls
    assert callable(BatchedMLP.tie_weights) and callable(BatchedMLP.take)
