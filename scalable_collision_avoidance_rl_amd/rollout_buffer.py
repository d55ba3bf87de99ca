"""On-device experience storage and its reductions.

The reference appends one namedtuple per agent and step to Python deques (`ExperienceBuffers`, utils.py:232-253,
called at train_problem.py:96) and scans them per agent at the end of the episode.  Here:

  RolloutStorage       utils.py:232-253        `[T, E, N, ...]` device tensors that the STEP KERNEL ITSELF fills:
                                               `drones.step(act, into=(storage, t))` hands slot t's addresses to
                                               `dronesim_step_ex`, so storing a transition costs no launch and no copy
  mc_returns           SAC_agents.py:304-307   G[t] = r[t] + gamma * G[t+1]
  lambda_returns       (no reference line)     TD(lambda) / GAE with a bootstrap from the value after the window's last step:
                                               G[t] = r[t] + gamma ((1 - lam) V[t+1] + lam G[t+1]), A = G - V
  episode_ends         (no reference line)     the kind of every episode end of an auto_reset window, from `z_final`: 1 terminal
                                               (arrival), 2 truncated (time limit), and the terminal observations of the
                                               truncated ones gathered for the critic; `lambda_returns(ends=, Vend=)` bootstraps
                                               a truncated end from the value of its terminal observation
  neighbour_advantage  SAC_agents.py:333-351   gamma^t / N * sum_{j in Ni[t]} (G_j[t] - V_i[t])

The reductions run in the HIP library (dronesim_returns / dronesim_lambda_returns / dronesim_episode_ends /
dronesim_lambda_returns_ends / dronesim_advantage); there is no CPU fallback."""
from __future__ import annotations

from collections import namedtuple

# the reference's experience tuple (utils.py:241-242), field for field
Experience = namedtuple("experience", ["z_state", "action", "reward", "next_z", "Ni", "finished"])


class RolloutStorage:
    """T steps of experience of a batched `drones` env, on its device, written by the step launches themselves.

    What `ExperienceBuffers.append(z_states, actions, rewards, new_z, Ni, finished)` (utils.py:244-249) stores per
    agent and step, as tensors over (step, env, agent):

        z_state  -> ``z_pre[t]``      the observation the action was based on   [T,E,N,(k+1)c]
        action   -> ``actions[t]``                                               [T,E,N,2]
        reward   -> ``reward[t]``     (+ ``true_reward[t]``, ``n_coll[t]``)      [T,E,N]
        next_z   -> ``next_z()[t]``   the observation after the step            [T,E,N,(k+1)c]
        Ni       -> ``nbr_pre[t]``    neighbour ids of ``z_pre`` (slot 0 = i, -1 = none)   [T,E,N,k+1]
        finished -> ``done[t]``                                                  [T,E]

    Observations live in ONE ring of T+1 slots: the step into slot t writes its new observation at ring index t+1, so
    ``z_pre`` (= ring[:T]) and the raw post-step observation ``z`` (= ring[1:]) are views of the same memory and the
    pre-step observation is never copied.  With ``auto_reset`` the post-step observation of a step that ends an episode
    is the NEW episode's first one (which is the right ``z_pre`` of the next step); the finished episode's terminal
    observation -- the reference's ``new_z`` for that transition (drone_env.py:258) -- is written by the same launch
    to ``z_final[t]`` / ``nbr_final[t]`` and merged by ``next_z()``.

        storage = RolloutStorage(env, T)
        storage.begin()                                   # slot 0 of the ring <- the env's current observation
        #                                                   (optional: a step into slot t carries the env's current
        #                                                   observation into ring slot t itself when it lives elsewhere,
        #                                                   e.g. after a manual `env.reset(mask=...)` between steps)
        for t in range(T):
            policy.sample_action(env.z, env=env, act_out=storage.actions[t])
            env.step(storage.actions[t], into=(storage, t))
        G = storage.returns(gamma); w = storage.advantage(storage.values, gamma)
    """

    def __init__(self, env, T, actions=True, values=False):
        import torch
        if not getattr(env, "batched", False):
            raise ValueError("RolloutStorage belongs to the batched (tensor) API of `drones`")
        self.env, self.T = env, int(T)
        E, N, K1, c = env.n_envs, env.n_agents, env.k_closest + 1, env.c
        dev = env.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.zbuf = torch.zeros(self.T + 1, E, N, K1 * c, **f32)
        self.nbrbuf = torch.full((self.T + 1, E, N, K1), -1, dtype=torch.int32, device=dev)
        self.reward = torch.zeros(self.T, E, N, **f32)
        self.true_reward = torch.zeros(self.T, E, N, **f32)
        self.n_coll = torch.zeros(self.T, E, dtype=torch.int32, device=dev)
        self.done = torch.zeros(self.T, E, dtype=torch.uint8, device=dev)
        self.actions = torch.zeros(self.T, E, N, 2, **f32) if actions else None
        self.values = torch.zeros(self.T, E, N, **f32) if values else None
        final = bool(env.auto_reset)
        self.z_final = torch.zeros(self.T, E, N, K1 * c, **f32) if final else None
        self.nbr_final = torch.full((self.T, E, N, K1), -1, dtype=torch.int32, device=dev) if final else None
        self._slots = [None] * self.T
        self._generation = None
        self.z_trunc = None                                  # `episode_ends` allocates its buffers on its first call
        self._ends = None

    # views over the observation ring
    z_pre = property(lambda self: self.zbuf[:self.T])
    nbr_pre = property(lambda self: self.nbrbuf[:self.T])
    z = property(lambda self: self.zbuf[1:])                 # raw post-step observation (new episode's first one after a reset)
    nbr_idx = property(lambda self: self.nbrbuf[1:])
    z_all = property(lambda self: self.zbuf)                 # all T+1 ring slots: z_all[T] is the observation after the window
    nbr_all = property(lambda self: self.nbrbuf)

    def begin(self):
        """Start (or restart) filling at slot 0: the env's current observation becomes ring slot 0 (ONE copy per T
        steps, none when the env is already bound there) and the env's observation attributes are bound to it."""
        env = self.env
        if env.z.data_ptr() != self.zbuf[0].data_ptr():
            self.zbuf[0].copy_(env.z)
            self.nbrbuf[0].copy_(env.nbr_idx)
        views = dict(reward=env.reward, true_reward=env.true_reward, z=self.zbuf[0], nbr_idx=self.nbrbuf[0],
                     n_coll=env.n_coll, done=env.done, z_final=env.z_final, nbr_final=env.nbr_final,
                     pos_final=env.pos_final)
        env._bind(views, home=False)
        return self

    def _slot(self, env, t):
        """(pre-marshalled DroneStepCall, attribute views) of slot t -- built once, reused by every later pass."""
        if env is not self.env:
            raise ValueError("this RolloutStorage belongs to another env")
        if not (0 <= t < self.T):
            raise IndexError(f"slot {t} outside a storage of {self.T} steps")
        gen = getattr(env, "_ctl_generation", 0)
        if gen != self._generation:                         # (load_state changed the seed the ctls carry)
            self._slots, self._generation = [None] * self.T, gen
        if self._slots[t] is None:
            zf = None if self.z_final is None else self.z_final[t]
            nf = None if self.nbr_final is None else self.nbr_final[t]
            views = dict(reward=self.reward[t], true_reward=self.true_reward[t], z=self.zbuf[t + 1],
                         nbr_idx=self.nbrbuf[t + 1], n_coll=self.n_coll[t], done=self.done[t],
                         z_final=zf, nbr_final=nf, pos_final=env._home["pos_final"],
                         actions=None if self.actions is None else self.actions[t],
                         _pre=(self.zbuf[t], self.nbrbuf[t], self.zbuf[t].data_ptr()))
            ctl = env._make_ctl(zf, nf, env._home["pos_final"]) if env._use_ctl else None
            env._params()
            self._slots[t] = (env._make_call(views, ctl), views)   # (the call keeps its ctl object alive)
        return self._slots[t]

    def next_z(self):
        """``new_z`` of every transition as the reference stores it (utils.py:244-249): the post-step observation,
        with the TERMINAL observation substituted where the step ended an episode under auto_reset.
        Returns ``(z [T,E,N,(k+1)c], nbr_idx [T,E,N,k+1])``."""
        import torch
        if self.z_final is None:
            return self.z, self.nbr_idx
        fin = self.done.bool()[:, :, None, None]
        return torch.where(fin, self.z_final, self.z), torch.where(fin, self.nbr_final, self.nbr_idx)

    def returns(self, gamma, true_rewards=False):
        """Monte-Carlo returns of the stored rewards, restarting at episode ends (`mc_returns`)."""
        return mc_returns(self.true_reward if true_rewards else self.reward, gamma, self.done)

    def lambda_returns(self, V, gamma, lam=1.0, true_rewards=False, want_adv=False, Vend=None):
        """Bootstrapped lambda-returns of the stored rewards (`lambda_returns`): ``V [T+1,E,N]`` are the critic's values of
        all ring slots, e.g. ``critic.forward(st.z_all.view((T+1)*E, N, -1)).view(T+1, E, N)``.  With ``Vend [M,E,N]``, the
        critic's values of ``z_trunc`` after `episode_ends` (same ``M``), a time-limit end bootstraps from the value of its
        terminal observation instead of being terminal."""
        reward = self.true_reward if true_rewards else self.reward
        if Vend is None:
            return lambda_returns(reward, V, gamma, lam, self.done, want_adv)
        if self._ends is None:
            raise ValueError("Vend needs the kinds of this window's episode ends: call episode_ends() first")
        return lambda_returns(reward, V, gamma, lam, None, want_adv, ends=self._ends[0], Vend=Vend)

    def episode_ends(self, M=None):
        """The kind of every episode end of the stored window (`episode_ends`): returns ``(ends [T,E] u8, slot_t [M,E] i32,
        n_trunc [E] i32)`` and fills ``self.z_trunc [M,E,N,(k+1)c]``, the terminal observations of the truncated (time-limit)
        ends ranked from the back of the window, zeros where there is none.  ``M`` defaults to ``ceil(T / max_time_steps)``:
        two time-limit ends of one env are at least ``max_time_steps`` slots apart.  The buffers are allocated on the first
        call (and again only when ``M`` changes); needs an env with ``auto_reset`` (``z_final``)."""
        import torch
        from . import drone_env
        if self.z_final is None:
            raise ValueError("episode_ends needs the terminal observations `z_final` of an env with auto_reset=True; "
                             "this storage has none")
        M = -(-self.T // drone_env.max_time_steps) if M is None else int(M)
        if M < 1:
            raise ValueError(f"M must be at least 1, got {M}")
        E = self.done.shape[1]
        if self._ends is None or self._ends[1].shape[0] != M:
            dev = self.done.device
            self._ends = (torch.empty_like(self.done), torch.empty(M, E, dtype=torch.int32, device=dev),
                          torch.empty(E, dtype=torch.int32, device=dev))
            self.z_trunc = torch.empty((M,) + tuple(self.z_final.shape[1:]), dtype=torch.float32, device=dev)
        _episode_ends(self.done, self.z_final, drone_env.DONE_RADIUS, M, *self._ends, self.z_trunc)
        return self._ends

    def safety(self, out=None):
        """The per-episode safety tables of the stored window (`evaluate.episode_safety`): closest approach, final goal
        distance and arrival step of every agent of every env's first episode, from the stored post-step observations (the
        terminal ones under auto_reset) and the env's live ``drone_radius`` / ``deltas``."""
        from .drone_env import DONE_RADIUS
        from .evaluate import episode_safety
        return episode_safety(self.z, self.nbr_idx, self.done, self.env._radius, self.env._delta, self.z_final, self.nbr_final,
                              DONE_RADIUS, out=out)

    def advantage(self, V, gamma, G=None):
        """Actor-loss weights from the stored pre-step neighbour lists (`neighbour_advantage`)."""
        G = self.returns(gamma) if G is None else G
        return neighbour_advantage(G, V, self.nbr_pre, gamma, self.done)

    def experience(self, t, i, e=0):
        """The reference's namedtuple for (step t, agent i) of env e, host-side (tests / debugging): flattened float64
        z rows, action, reward, next_z, ``Ni`` as the reference's list (i first, ghost slots dropped), finished."""
        nz, _ = self.next_z()
        nb = self.nbr_pre[t, e, i].cpu().numpy()
        act = None if self.actions is None else self.actions[t, e, i].double().cpu().numpy()
        return Experience(self.z_pre[t, e, i].double().cpu().numpy(), act, float(self.reward[t, e, i]),
                          nz[t, e, i].double().cpu().numpy(), [int(j) for j in nb if j >= 0], bool(self.done[t, e]))

    def __len__(self):
        return self.T



def _prep(x, dtype, shape=None):
    import torch
    if not (torch.is_tensor(x) and x.is_cuda):
        raise RuntimeError("rollout_buffer works on ROCm device tensors only (no CPU fallback)")
    x = x.to(dtype).contiguous()
    if shape is not None and tuple(x.shape) != tuple(shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {tuple(x.shape)}")
    return x


def mc_returns(reward, gamma: float, done=None):
    """Monte-Carlo returns of every (env, agent) column of ``reward [T,E,N]``; ``done [T,E]`` (optional)
    marks steps that ended an episode (the scan restarts there)."""
    import torch
    from . import _native
    reward = _prep(reward, torch.float32)
    T, E, N = reward.shape
    d = None if done is None else _prep(done, torch.uint8, (T, E))
    G = torch.empty_like(reward)
    _native.call("dronesim_returns", reward, d, float(gamma), G, T, E, N)
    return G


def check_lam(lam):
    """``lam`` as a float in [0, 1], else ValueError (numbers only: no strings, no NaN)."""
    import numbers
    if isinstance(lam, bool) or not isinstance(lam, numbers.Real) or not 0.0 <= float(lam) <= 1.0:
        raise ValueError(f"lam must be a number in [0, 1], got {lam!r}")
    return float(lam)


def _episode_ends(done, z_final, done_radius, M, ends, slot_t, n_trunc, z_trunc):
    """`dronesim_episode_ends` on checked, contiguous device tensors, into the caller's buffers."""
    from . import _native
    T, E, N, d = z_final.shape
    _native.call("dronesim_episode_ends", done, z_final, T, E, N, d, float(done_radius), ends, slot_t, n_trunc, z_trunc, M)


def episode_ends(done, z_final, done_radius, M):
    """The kind of every episode end of a stored auto_reset window, from the window itself: ``done [T,E]`` (u8) and the
    terminal observations ``z_final [T,E,N,d]`` whose rows start with the agent's own offset (zx, zy) from its goal.

        ends [T,E] u8        0 no end, 1 terminal (done, every agent within ``done_radius``), 2 truncated (done with some agent
                             outside: the time limit -- an arrival on the last allowed step is terminal)
        slot_t [M,E] i32     t of env e's k-th truncated end counted from the BACK of the window, -1 where there is none
        n_trunc [E] i32      the env's truncated ends (an end with k >= M is demoted to ends = 1: ``n_trunc > M`` tells)
        z_trunc [M,E,N,d]    z_final[slot_t[k,e], e], zeros where slot_t is -1

    Returns ``(ends, slot_t, n_trunc, z_trunc)``.  The test is the step kernel's own, ``!(sqrt(zx^2 + zy^2) <= done_radius)``
    in float32: a non-finite offset counts as outside."""
    import torch
    if not (torch.is_tensor(done) and torch.is_tensor(z_final)) or z_final.dim() != 4 or z_final.shape[3] < 2 or \
            tuple(done.shape) != tuple(z_final.shape[:2]):
        raise ValueError(f"done must be [T,E] and z_final [T,E,N,d] with d >= 2, got "
                         f"{tuple(getattr(done, 'shape', ()))} and {tuple(getattr(z_final, 'shape', ()))}")
    if isinstance(M, bool) or int(M) != M or M < 1:
        raise ValueError(f"M must be an integer >= 1, got {M!r}")
    M = int(M)
    z_final = _prep(z_final, torch.float32)
    T, E, N, d = z_final.shape
    done = _prep(done, torch.uint8, (T, E))
    dev = done.device
    out = (torch.empty_like(done), torch.empty(M, E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.int32, device=dev),
           torch.empty(M, E, N, d, dtype=torch.float32, device=dev))
    _episode_ends(done, z_final, done_radius, M, *out)
    return out


def lambda_returns(reward, V, gamma: float, lam: float = 1.0, done=None, want_adv=False, ends=None, Vend=None):
    """TD(lambda) returns of every (env, agent) column of ``reward [T,E,N]`` for a window that may cut episodes:
    ``V [T+1,E,N]`` holds the value of the observation each step acted on and, in its last slot, of the observation after
    the last step, from which the scan bootstraps; ``done [T,E]`` (optional) marks steps that ended an episode -- terminal,
    nothing is carried across them.  ``lam = 1`` is Monte-Carlo plus the bootstrap at the window's end, ``lam = 0`` the
    one-step target.  Returns ``G``, or ``(G, A)`` with the GAE(gamma, lam) advantage ``A = G - V[:T]`` when ``want_adv``.

    ``ends [T,E]`` (u8) and ``Vend [M,E,N]`` -- both or neither -- replace ``done`` by the KIND of every end (`episode_ends`):
    1 is terminal as above; 2, a time-limit end, gives ``G[t] = r[t] + gamma Vend[k]`` with k the number of the env's
    truncated ends at later t (terminal once k reaches M), whatever ``lam`` is.  ``done`` is not read then."""
    import torch
    if (ends is None) != (Vend is None):
        raise ValueError("ends and Vend go together: the kinds of the episode ends [T,E] and the values [M,E,N] of the "
                         "terminal observations of the truncated ones (episode_ends); got only one of them")
    from . import _native
    lam = check_lam(lam)
    if torch.is_tensor(reward) and torch.is_tensor(V) and (
            reward.dim() != 3 or tuple(V.shape) != (reward.shape[0] + 1,) + tuple(reward.shape[1:])):
        raise ValueError(f"reward must be [T,E,N] and V [T+1,E,N] (one more leading slot: the value after the last step), "
                         f"got {tuple(reward.shape)} and {tuple(V.shape)}")
    if ends is not None and torch.is_tensor(reward) and reward.dim() == 3:
        if not torch.is_tensor(Vend) or Vend.dim() != 3 or Vend.shape[0] < 1 or tuple(Vend.shape[1:]) != tuple(reward.shape[1:]):
            raise ValueError(f"Vend must be [M,E,N] = [M >= 1, {reward.shape[1]}, {reward.shape[2]}], "
                             f"got {tuple(getattr(Vend, 'shape', ()))}")
        if not torch.is_tensor(ends) or tuple(ends.shape) != tuple(reward.shape[:2]):
            raise ValueError(f"ends must be [T,E] = {tuple(reward.shape[:2])}, got {tuple(getattr(ends, 'shape', ()))}")
    reward = _prep(reward, torch.float32)
    T, E, N = reward.shape
    V = _prep(V, torch.float32, (T + 1, E, N))
    if ends is not None:
        ends, Vend = _prep(ends, torch.uint8, (T, E)), _prep(Vend, torch.float32)
        G = torch.empty_like(reward)
        A = torch.empty_like(reward) if want_adv else None
        _native.call("dronesim_lambda_returns_ends", reward, ends, V, Vend, int(Vend.shape[0]), float(gamma), lam, G, A, T, E, N)
        return (G, A) if want_adv else G
    d = None if done is None else _prep(done, torch.uint8, (T, E))
    G = torch.empty_like(reward)
    A = torch.empty_like(reward) if want_adv else None
    _native.call("dronesim_lambda_returns", reward, d, V, float(gamma), lam, G, A, T, E, N)
    return (G, A) if want_adv else G


def neighbour_advantage(G, V, nbr_idx, gamma: float, done=None):
    """Actor-loss weight ``gamma^t / N * sum_{j in Ni} (G_j - V_i)`` for ``G, V [T,E,N]`` and the neighbour
    lists ``nbr_idx [T,E,N,k+1]`` the actions were based on (the PRE-step observation: `env.nbr_idx`
    before each step, i.e. ``rollout()['nbr_idx_pre']``)."""
    import torch
    from . import _native
    G = _prep(G, torch.float32)
    T, E, N = G.shape
    V = _prep(V, torch.float32, (T, E, N))
    nbr_idx = _prep(nbr_idx, torch.int32)
    if nbr_idx.dim() != 4 or tuple(nbr_idx.shape[:3]) != (T, E, N):
        raise ValueError(f"nbr_idx must be [T,E,N,k+1], got {tuple(nbr_idx.shape)}")
    d = None if done is None else _prep(done, torch.uint8, (T, E))
    w = torch.empty_like(G)
    _native.call("dronesim_advantage", G, V, nbr_idx, d, float(gamma), w, T, E, N, int(nbr_idx.shape[3]))
    return w


def standardize(x, eps=1e-8, out=None, return_stats=False):
    """Per-agent standardisation of ``x [..., N]`` (e.g. a window's advantages ``[T,E,N]``) over all leading axes:
    ``(x - mean_i) / (std_i + eps)`` with float64 sums and the population std (`dronesim_standardize`; deterministic, no host
    synchronisation).  ``out``: a contiguous float32 tensor of x's shape to write into (``out=x`` works in place).  Returns
    ``y``, or ``(y, stats)`` with ``stats [2, N]`` = (mean, std) of the input when ``return_stats``."""
    import torch
    from . import _native
    x = _prep(x, torch.float32)
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"x must be a non-empty [..., N] tensor, got shape {tuple(x.shape)}")
    N = int(x.shape[-1])
    R = x.numel() // N
    if isinstance(eps, bool) or not eps >= 0:
        raise ValueError(f"eps must be a number >= 0, got {eps!r}")
    if out is None:
        out = torch.empty_like(x)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
              and tuple(out.shape) == tuple(x.shape)):
        raise ValueError(f"out must be a contiguous float32 device tensor of shape {tuple(x.shape)}")
    ws_bytes = _native.workspace("dronesim_standardize_workspace", R, N)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=x.device)
    stats = torch.empty(2, N, dtype=torch.float32, device=x.device) if return_stats else None
    _native.call("dronesim_standardize", x, out, stats, R, N, float(eps), ws, ws_bytes)
    return (out, stats) if return_stats else out
