"""Host-side tests of the bootstrapped lambda-returns (TD(lambda) / GAE): the float64 restatement (tests/lambda_ref.py)
against the definition and its identities, the new entry point's ABI and argument validation, and the learners' and the
storage face's host logic (no GPU needed)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from scalable_collision_avoidance_rl_amd import _native
from tests import lambda_ref as L
from tests import learner_ref as R
from tests.test_ppo_host import host_mlp

NAME = "dronesim_lambda_returns"


def window(gen, T, E, N, p_done=0.15):
    reward = torch.randn(T, E, N, generator=gen, dtype=torch.float64) * 3
    V = torch.randn(T + 1, E, N, generator=gen, dtype=torch.float64) * 5
    done = (torch.rand(T, E, generator=gen) < p_done).to(torch.uint8)
    return reward, V, done


def test_recurrence_equals_the_definition_on_random_windows():
    """A[t] = sum_l (gamma lam)^l delta[t+l] stopped at the first done, delta = r + gamma (1 - done) V[t+1] - V[t]."""
    gen = torch.Generator().manual_seed(11)
    for it in range(25):
        T = int(torch.randint(1, 41, (1,), generator=gen))
        E, N = int(torch.randint(1, 5, (1,), generator=gen)), int(torch.randint(1, 4, (1,), generator=gen))
        gamma = 0.5 + 0.5 * float(torch.rand(1, generator=gen))
        lam = (0.0, 1.0, 0.5, 0.95, float(torch.rand(1, generator=gen)))[it % 5]
        reward, V, done = window(gen, T, E, N)
        d = None if it % 4 == 3 else done
        G, A = L.lambda_returns(reward, V, d, gamma, lam)
        Gb, Ab = L.brute_force(reward, V, d, gamma, lam)
        scale = float(torch.maximum(reward.abs().max(), V.abs().max())) * T
        np.testing.assert_allclose(A.numpy(), Ab.numpy(), rtol=1e-12, atol=1e-12 * scale, err_msg=f"A {it} T={T} lam={lam}")
        np.testing.assert_allclose(G.numpy(), Gb.numpy(), rtol=1e-12, atol=1e-12 * scale, err_msg=f"G {it} T={T} lam={lam}")
        assert torch.equal(A, G - V[:T])


def test_identities_at_lam_zero_and_one():
    gen = torch.Generator().manual_seed(12)
    T, E, N, gamma = 23, 6, 3, 0.93
    reward, V, done = window(gen, T, E, N)
    # lam = 0: the one-step target
    G0, _ = L.lambda_returns(reward, V, done, gamma, 0.0)
    np.testing.assert_allclose(G0.numpy(), (reward + gamma * (1 - done.double())[:, :, None] * V[1:]).numpy(), rtol=1e-14, atol=0)
    # lam = 1, the window's last step done everywhere: the Monte-Carlo returns, whatever V is
    dl = done.clone(); dl[T - 1] = 1
    G1, _ = L.lambda_returns(reward, V, dl, gamma, 1.0)
    np.testing.assert_allclose(G1.numpy(), R.returns(reward, dl, gamma).numpy(), rtol=1e-13, atol=1e-13)
    # lam = 1, no done: Monte-Carlo plus gamma^(T-t) V[T]
    none = torch.zeros_like(done)
    for d in (none, None):
        Gb, _ = L.lambda_returns(reward, V, d, gamma, 1.0)
        tail = gamma ** torch.arange(T, 0, -1, dtype=torch.float64)[:, None, None] * V[T]
        np.testing.assert_allclose(Gb.numpy(), (R.returns(reward, none, gamma) + tail).numpy(), rtol=1e-13, atol=1e-13)


def test_library_exports_the_entry_point_with_the_declared_argtypes():
    lib = _native.lib()
    assert NAME in _native.SYMBOLS
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int
    assert f"int {NAME}(" in open(_native.HEADER_PATH).read()
    assert lib.dronesim_version() == 600


OK_ARGS = dict(reward=4096, done=4096, V=4096, gamma=0.99, lam=0.95, G=4096, A=4096, T=4, E=2, N=5)


def test_entry_point_rejects_bad_arguments_on_the_host():
    """Every EINVAL case is decided before anything is enqueued: the dummy addresses are never dereferenced."""
    lib = _native.lib()
    call = lambda **kw: lib.dronesim_lambda_returns(*{**OK_ARGS, **kw}.values(), None)
    nan = float("nan")
    for bad in (dict(reward=None), dict(V=None), dict(G=None, A=None), dict(T=-1), dict(E=-1), dict(N=0), dict(N=-3),
                dict(lam=-0.1), dict(lam=1.5), dict(lam=nan), dict(gamma=nan), dict(lam=float("inf"))):
        assert call(**bad) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(NAME.encode()), bad
    # an empty window enqueues nothing (one output or no done flags are fine)
    assert call(T=0) == _native.OK and call(E=0) == _native.OK
    assert call(T=0, G=None) == _native.OK and call(E=0, A=None, done=None) == _native.OK


def test_quadruple_rule_at_its_edges():
    """The one host helper behind the four entry points (csrc/scan_common.hpp: column_quads) against the expressions they each
    carried: agents in fours, every base 16-byte aligned, 262144 <= columns < the caller's bound (1048576 for
    dronesim_returns / dronesim_episode_eval, 524288 for the two lambda scans)."""
    fn = _native.lib().dronesim_debug_column_quads
    fn.argtypes, fn.restype = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64], C.c_int
    base = 0x7F0000001000
    for upper in (1048576, 524288):
        for cols in (262140, 262144, 524284, 524288, 1048572, 1048576):
            for N in (3, 4):
                for addresses in (base, base | (base + 4), base | (base + 16), 0):
                    old = N % 4 == 0 and (addresses & 15) == 0 and cols >= 262144 and cols < upper
                    assert fn(N, cols, upper, addresses) == int(old), (N, cols, upper, hex(addresses))
    assert fn(4, 262144, 524288, base) == 1 and fn(4, 262140, 524288, base) == 0          # the lower bound, everywhere
    assert fn(4, 524284, 524288, base) == 1 and fn(4, 524288, 524288, base) == 0          # the lambda scans' upper bound
    assert fn(4, 524288, 1048576, base) == 1 and fn(4, 1048572, 1048576, base) == 1 and fn(4, 1048576, 1048576, base) == 0
    assert fn(3, 262144, 1048576, base) == 0 and fn(4, 262144, 1048576, base | (base + 4)) == 0


GOOD_LAM, BAD_LAM = (None, 0.0, 1.0, 0.95), (-0.1, 1.5, float("nan"), "1")


@pytest.mark.parametrize("which", ["sa2c", "ppo"])
def test_learners_validate_lam_and_need_the_observation_ring(which):
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner, SA2CLearner
    cls = SA2CLearner if which == "sa2c" else PPOLearner
    actor, critic = host_mlp(1, 16), host_mlp(0, 1)
    assert cls(actor, critic, 0.99).lam is None
    for lam in GOOD_LAM:
        assert cls(actor, critic, 0.99, lam=lam).lam == lam
    for lam in BAD_LAM:
        with pytest.raises(ValueError, match="lam"):
            cls(actor, critic, 0.99, lam=lam)
    # a storage-like object without the T+1-slot ring
    st = SimpleNamespace(z_pre=torch.zeros(4, 2, 3, 6), reward=torch.zeros(4, 2, 3), done=torch.zeros(4, 2, dtype=torch.uint8),
                         actions=torch.zeros(4, 2, 3, 2), nbr_pre=torch.zeros(4, 2, 3, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="z_all"):
        cls(actor, critic, 0.99, lam=0.95).train(st)
    st.z_all = torch.zeros(4, 2, 3, 6)                       # T slots where T + 1 are needed
    with pytest.raises(ValueError, match="z_all"):
        cls(actor, critic, 0.99, lam=0.95).train(st)


def test_python_face_validates_on_the_host_and_has_no_cpu_fallback():
    import scalable_collision_avoidance_rl_amd as pkg
    from scalable_collision_avoidance_rl_amd import rollout_buffer as RB
    assert pkg.lambda_returns is RB.lambda_returns and "lambda_returns" in pkg.__all__
    r, V = torch.zeros(4, 2, 3), torch.zeros(5, 2, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RB.lambda_returns(r, V, 0.99, 0.95)
    for lam in BAD_LAM:
        with pytest.raises(ValueError, match="lam"):
            RB.lambda_returns(r, V, 0.99, lam)
    for bad_V in (torch.zeros(4, 2, 3), torch.zeros(6, 2, 3), torch.zeros(5, 2, 4), torch.zeros(5, 6)):
        with pytest.raises(ValueError, match="one more leading slot"):
            RB.lambda_returns(r, bad_V, 0.99, 0.95)
    assert hasattr(RB.RolloutStorage, "z_all") and hasattr(RB.RolloutStorage, "nbr_all") and hasattr(RB.RolloutStorage, "lambda_returns")
