"""Host-side tests of the time-limit handling of the bootstrapped lambda-returns: the numpy restatement
(tests/timelimit_ref.py) against an independent reading of its definition, the two new entry points' ABI and argument
validation, and the host logic of the new Python arguments (no GPU needed)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from scalable_collision_avoidance_rl_amd import _native
from tests import lambda_ref as L
from tests import timelimit_ref as TL
from tests.test_ppo_host import host_mlp

ENDS, SCAN = "dronesim_episode_ends", "dronesim_lambda_returns_ends"


def random_window(rng, T, E, N, M, p=(0.85, 0.08, 0.07)):
    reward = rng.standard_normal((T, E, N)) * 3
    V = rng.standard_normal((T + 1, E, N)) * 5
    Vend = rng.standard_normal((M, E, N)) * 5
    ends = rng.choice(3, size=(T, E), p=p).astype(np.uint8)
    return reward, V, ends, Vend


def by_segments(reward, V, ends, Vend, gamma, lam):
    """The definition read column by column: cut every env's window at its ends and hand each segment on its own to
    `lambda_ref.lambda_returns` as a window without done, with the value after its last step := the segment's Vend for a
    truncated end, 0 together with a final done for a terminal end, the real V[T] for the segment the window cuts."""
    T, E, N = reward.shape
    M = Vend.shape[0]
    G = np.zeros((T, E, N))
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    for e in range(E):
        stops = [t for t in range(T) if ends[t, e] != 0]
        n2 = sum(1 for t in stops if ends[t, e] == 2)
        k_of, seen = {}, 0
        for t in stops:                                     # k = number of truncated ends at LATER t
            if ends[t, e] == 2:
                seen += 1
                k_of[t] = n2 - seen
        a = 0
        for b in stops + ([T - 1] if not stops or stops[-1] != T - 1 else []):
            n = b + 1 - a
            done = None
            if ends[b, e] == 2 and k_of[b] < M:
                last = Vend[k_of[b], e]
            elif ends[b, e] != 0:                           # terminal, or truncated beyond the capacity
                last = np.zeros(N)
                done = torch.zeros(n, 1, dtype=torch.uint8)
                done[n - 1] = 1
            else:
                last = V[T, e]
            Vseg = np.concatenate([V[a:b + 1, e], last[None]], 0)[:, None, :]
            g, _ = L.lambda_returns(tt(reward[a:b + 1, e][:, None, :]), tt(Vseg), done, gamma, lam)
            G[a:b + 1, e] = g[:, 0].numpy()
            a = b + 1
    return G, G - V[:T]


@pytest.mark.parametrize("gamma", [1.0, 0.97])
@pytest.mark.parametrize("lam", [0.0, 0.5, 0.95, 1.0])
def test_scan_restatement_equals_the_segments_of_the_definition(lam, gamma):
    rng = np.random.default_rng(int(lam * 100) * 7 + int(gamma * 100))
    for it in range(12):
        T, E, N, M = int(rng.integers(1, 41)), int(rng.integers(1, 6)), int(rng.integers(1, 4)), int(rng.integers(1, 4))
        reward, V, ends, Vend = random_window(rng, T, E, N, M, p=(0.7, 0.12, 0.18) if it % 2 else (0.85, 0.08, 0.07))
        if it == 0:
            ends[T - 1] = 2                                 # an end on the window's last step
        G, A = TL.lambda_returns_ends(reward, V, ends, Vend, gamma, lam)
        Gs, As = by_segments(reward, V, ends, Vend, gamma, lam)
        scale = max(np.abs(reward).max(), np.abs(V).max(), np.abs(Vend).max()) * T
        np.testing.assert_allclose(G, Gs, rtol=1e-12, atol=1e-12 * scale, err_msg=f"G {it} T={T} M={M}")
        np.testing.assert_allclose(A, As, rtol=1e-12, atol=1e-12 * scale, err_msg=f"A {it} T={T} M={M}")


def test_scan_restatement_without_truncated_ends_is_the_lambda_restatement():
    rng = np.random.default_rng(3)
    reward, V, ends, Vend = random_window(rng, 23, 6, 3, 2, p=(0.85, 0.15, 0.0))
    G, A = TL.lambda_returns_ends(reward, V, ends, Vend, 0.97, 0.9)
    Gl, Al = L.lambda_returns(torch.from_numpy(reward), torch.from_numpy(V), torch.from_numpy(ends), 0.97, 0.9)
    np.testing.assert_allclose(G, Gl.numpy(), rtol=1e-14, atol=0)
    np.testing.assert_allclose(A, Al.numpy(), rtol=1e-13, atol=1e-13)


def test_a_truncated_end_does_not_depend_on_lam():
    rng = np.random.default_rng(4)
    reward, V, ends, Vend = random_window(rng, 9, 4, 3, 1)
    ends[:] = 0
    ends[8] = 2
    for lam in (0.0, 0.3, 1.0):
        G, _ = TL.lambda_returns_ends(reward, V, ends, Vend, 0.97, lam)
        assert np.array_equal(G[8], reward[8] + 0.97 * Vend[0])


def test_classification_ranking_demotion_and_zero_fill():
    """A hand-made window: T = 6, E = 4, N = 2, d = 3, radius 0.2."""
    T, E, N, d = 6, 4, 2, 3
    z = np.full((T, E, N, d), 7.0, np.float32)
    z[..., :2] = 0.01                                       # every agent inside ...
    done = np.zeros((T, E), np.uint8)
    done[[0, 2, 5], 0] = 1; z[0, 0, 1, 0] = 0.5; z[2, 0, 0, 1] = -0.3; z[5, 0, 1, :2] = (0.15, 0.15)   # env 0: three truncated
    done[3, 1] = 1                                          # env 1: an arrival
    done[1, 2] = 1; z[1, 2, 0, 0] = np.nan                  # env 2: a NaN offset is outside
    z[4, 3, :, 0] = 9.0                                     # env 3: outside but not done
    ends, slot_t, n_trunc, z_trunc = TL.episode_ends(done, z, 0.2, 2)
    assert ends[:, 0].tolist() == [1, 0, 2, 0, 0, 2]        # the earliest of the three is demoted (k = 2 >= M)
    assert ends[:, 1].tolist() == [0, 0, 0, 1, 0, 0] and ends[:, 2].tolist() == [0, 2, 0, 0, 0, 0] and not ends[:, 3].any()
    assert slot_t.tolist() == [[5, -1, 1, -1], [2, -1, -1, -1]] and n_trunc.tolist() == [3, 0, 1, 0]
    assert np.array_equal(z_trunc[0, 0], z[5, 0]) and np.array_equal(z_trunc[1, 0], z[2, 0])
    assert np.array_equal(z_trunc[0, 2], z[1, 2], equal_nan=True)
    assert not z_trunc[:, 1].any() and not z_trunc[:, 3].any() and not z_trunc[1, 2].any()
    ends1, slot1, n1, _ = TL.episode_ends(done, z, 0.2, 1)
    assert ends1[:, 0].tolist() == [1, 0, 1, 0, 0, 2] and slot1.tolist() == [[5, -1, 1, -1]] and n1.tolist() == [3, 0, 1, 0]


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_library_exports_the_entry_points_with_the_declared_argtypes():
    lib = _native.lib()
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    header = open(_native.HEADER_PATH).read()
    for name in (ENDS, SCAN):
        assert name in _native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int
        assert f"int {name}(" in header
    # the header's parameter lists, type by type, against the argtypes
    kinds = {"const uint8_t *": vp, "const float *": vp, "uint8_t *": vp, "int32_t *": vp, "float *": vp, "void *": vp,
             "int ": i32, "float ": f32}
    for name in (ENDS, SCAN):
        params = header.split(f"int {name}(")[1].split(")")[0].replace("\n", " ").split(",")
        got = [next(v for k, v in kinds.items() if p.strip().startswith(k)) for p in params]
        assert got == list(getattr(lib, name).argtypes), name


ENDS_OK = dict(done=4096, z_final=4096, T=4, E=2, N=5, d=6, done_radius=0.2, ends=4096, slot_t=4096, n_trunc=4096, z_trunc=4096, M=1)
SCAN_OK = dict(reward=4096, ends=4096, V=4096, Vend=4096, M=1, gamma=0.99, lam=0.95, G=4096, A=4096, T=4, E=2, N=5)


def test_entry_points_reject_bad_arguments_on_the_host():
    """Every EINVAL case is decided before anything is enqueued: the dummy addresses are never dereferenced."""
    lib = _native.lib()
    nan = float("nan")
    call = lambda **kw: lib.dronesim_episode_ends(*{**ENDS_OK, **kw}.values(), None)
    for bad in (dict(done=None), dict(z_final=None), dict(ends=None), dict(slot_t=None), dict(n_trunc=None), dict(z_trunc=None),
                dict(T=-1), dict(E=-1), dict(N=0), dict(d=1), dict(M=0), dict(M=-2), dict(done_radius=nan)):
        assert call(**bad) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(ENDS.encode()), bad
    assert call(E=0) == _native.OK
    call = lambda **kw: lib.dronesim_lambda_returns_ends(*{**SCAN_OK, **kw}.values(), None)
    for bad in (dict(reward=None), dict(V=None), dict(ends=None), dict(Vend=None), dict(G=None, A=None), dict(T=-1), dict(E=-1),
                dict(N=0), dict(M=0), dict(M=-1), dict(lam=-0.1), dict(lam=1.5), dict(lam=nan), dict(gamma=nan)):
        assert call(**bad) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(SCAN.encode()), bad
    assert call(T=0) == _native.OK and call(E=0) == _native.OK and call(T=0, G=None) == _native.OK


# ------------------------------------------------------------------------------------------------------ the Python arguments
@pytest.mark.parametrize("which", ["sa2c", "ppo"])
def test_learners_validate_time_limit(which):
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner, SA2CLearner
    cls = SA2CLearner if which == "sa2c" else PPOLearner
    actor, critic = host_mlp(1, 16), host_mlp(0, 1)
    assert cls(actor, critic, 0.99).time_limit == "terminal" and cls(actor, critic, 0.99, lam=0.9).time_limit == "terminal"
    assert cls(actor, critic, 0.99, lam=0.95, time_limit="bootstrap").time_limit == "bootstrap"
    assert cls(actor, critic, 0.99, time_limit="terminal").lam is None
    with pytest.raises(ValueError, match="lam"):
        cls(actor, critic, 0.99, time_limit="bootstrap")
    for bad in ("truncate", "", None, 1, "Bootstrap"):
        with pytest.raises(ValueError, match="time_limit"):
            cls(actor, critic, 0.99, lam=0.95, time_limit=bad)
    # a storage-like object with the ring but without z_final (an env without auto_reset)
    st = SimpleNamespace(z_pre=torch.zeros(4, 2, 3, 6), reward=torch.zeros(4, 2, 3), done=torch.zeros(4, 2, dtype=torch.uint8),
                         actions=torch.zeros(4, 2, 3, 2), nbr_pre=torch.zeros(4, 2, 3, 3, dtype=torch.int32),
                         z_all=torch.zeros(5, 2, 3, 6))
    with pytest.raises(ValueError, match="z_final"):
        cls(actor, critic, 0.99, lam=0.95, time_limit="bootstrap").train(st)
    st.z_final = torch.zeros(4, 2, 3, 5)
    with pytest.raises(ValueError, match="z_final"):
        cls(actor, critic, 0.99, lam=0.95, time_limit="bootstrap").train(st)


def test_python_face_validates_on_the_host():
    import scalable_collision_avoidance_rl_amd as pkg
    from scalable_collision_avoidance_rl_amd import rollout_buffer as RB
    assert pkg.episode_ends is RB.episode_ends and "episode_ends" in pkg.__all__
    r, V = torch.zeros(4, 2, 3), torch.zeros(5, 2, 3)
    ends, Vend = torch.zeros(4, 2, dtype=torch.uint8), torch.zeros(1, 2, 3)
    with pytest.raises(ValueError, match="go together"):
        RB.lambda_returns(r, V, 0.99, 0.95, ends=ends)
    with pytest.raises(ValueError, match="go together"):
        RB.lambda_returns(r, V, 0.99, 0.95, Vend=Vend)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RB.lambda_returns(r, V, 0.99, 0.95, ends=ends, Vend=Vend)
    for bad in (torch.zeros(2, 3), torch.zeros(1, 2, 4), torch.zeros(1, 3, 3), torch.zeros(0, 2, 3)):
        with pytest.raises(ValueError, match="Vend"):
            RB.lambda_returns(r, V, 0.99, 0.95, ends=ends, Vend=bad)
    done, zf = torch.zeros(4, 2, dtype=torch.uint8), torch.zeros(4, 2, 3, 6)
    for d_, z_ in ((done, zf[0]), (done[:3], zf), (done, torch.zeros(4, 2, 3, 1)), (done.T, zf)):
        with pytest.raises(ValueError, match="z_final"):
            RB.episode_ends(d_, z_, 0.2, 1)
    for M in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="M must"):
            RB.episode_ends(done, zf, 0.2, M)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RB.episode_ends(done, zf, 0.2, 1)
    assert hasattr(RB.RolloutStorage, "episode_ends")
