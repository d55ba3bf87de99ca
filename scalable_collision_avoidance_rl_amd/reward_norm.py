"""Reward normalisation: a reward scale from the running discounted return, kept and applied on the device.

The reward is ``-(0.1 |x - xF|^2 + b sum log-terms)``: its size grows with the square of the grid's side, and a return adds up
to 200 such terms -- O(10^2) at G = 5, O(10^4) at 28, O(10^6) at 256.  `ObsNormalizer` makes the networks' inputs O(1) at any
grid; `RewardNormalizer` does the same for their targets, the usual way: every (env, agent) column carries the discounted
return ``R <- gamma R + r`` (reset behind ``done``) across windows, the R of every step go into per-group running moments
(csrc/rewnorm.hip: float64, Chan's merge, one fixed order), and rewards are multiplied by ``1 / sqrt(var(R) + eps)``.  No mean
is subtracted.

    rnorm = RewardNormalizer(env.n_agents, gamma, env.device)
    learner = PPOLearner(actor, critic, gamma, reward_norm=rnorm)     # train() merges the window, then scales it

  update(reward, done)   dronesim_rewnorm_update   scan ``reward [T,E,N]`` / ``done [T,E]`` forward, merge the finite returns
                                                   into the state, rewrite the scale
  norm(reward)           dronesim_rewnorm_apply    ``reward * scale``, clamped to ``[-clip, clip]``; NaN stays NaN

Only finite returns are counted.  A NaN or +-inf reward poisons its column's carry until that column's next ``done``; those
steps are not counted and the carry is not repaired.

``scope`` says which agents share one scale: ``"team"`` (default) all of them -- both learners' advantages add the returns of an
agent's neighbours, and a sum needs one unit --, ``"agent"`` one group per agent, or a sharing map (whatever
`learner.agent_groups` accepts) one group per tied group.

Both calls enqueue kernels only -- no host synchronisation, no memset node, nothing allocated after the first call per shape --
so a rollout window and ``train()`` replay from one captured graph.  Importing this module needs neither a GPU nor the built
library; `update` and `norm` need both (no CPU fallback).  A normaliser on the CPU only carries statistics (`state_dict`)."""
from __future__ import annotations

import math

from .obs_norm import _check_clip

SCOPES = ("team", "agent")


def _groups(scope, n_agents):
    """``(group_of [N], n_groups)`` of a ``scope``: "team", "agent" or a sharing map."""
    from .learner import agent_groups
    if isinstance(scope, str):
        if scope not in SCOPES:
            raise ValueError(f'scope must be one of {SCOPES} or a sequence of {n_agents} group ids, got {scope!r}')
        scope = "all" if scope == "team" else None
    elif scope is None:
        raise ValueError(f'scope must be one of {SCOPES} or a sequence of {n_agents} group ids, got None')
    group_of, ptr, _ = agent_groups(scope, n_agents)
    return group_of, len(ptr) - 1


def scale_of_state(state, eps):
    """``scale [G]`` of a ``state [3,G]`` (float64, host side): ``1 / sqrt(m2 / count + eps)``, and 1 where the count is 0 or
    that denominator is 0."""
    import torch
    n, m2 = state[0], state[2]
    var = torch.where(n > 0, m2 / n.clamp(min=1.0) + eps, torch.zeros_like(n))
    return torch.where(var > 0, 1.0 / torch.sqrt(torch.where(var > 0, var, torch.ones_like(var))), torch.ones_like(var))


class RewardNormalizer:
    """Running moments of the discounted return per statistics group.  ``state [3,G]`` = (count, mean, m2), ``scale [N]`` (agent
    i's entry is its group's scale) and the carry ``ret [E,N]`` (made at the first `update`) are float64 tensors on ``device``
    that only the kernels write; a fresh normaliser holds scale 1.  ``clip=None``: no clamp."""

    def __init__(self, n_agents, gamma, device, scope="team", clip=10.0, eps=1e-8):
        import numbers
        import torch
        if isinstance(n_agents, bool) or not isinstance(n_agents, numbers.Integral) or n_agents < 1:
            raise ValueError(f"n_agents must be an integer >= 1, got {n_agents!r}")
        if isinstance(gamma, bool) or not isinstance(gamma, numbers.Real) or not 0.0 <= gamma <= 1.0:
            raise ValueError(f"gamma must be a number in [0, 1], got {gamma!r}")
        if isinstance(eps, bool) or not isinstance(eps, numbers.Real) or not math.isfinite(eps) or eps < 0:
            raise ValueError(f"eps must be a finite number >= 0, got {eps!r}")
        self.n_agents, self.gamma, self.device = int(n_agents), float(gamma), torch.device(device)
        self.clip, self.eps = _check_clip(clip), float(eps)
        self._set_groups(*_groups(scope, self.n_agents))
        self.ret = None
        self._ws = None
        self._ws_bytes = {}                 # (T, E) -> workspace bytes
        self._out = {}                      # input shape -> the owned output buffer of `norm`

    def _set_groups(self, group_of, n_groups):
        import torch
        self.group_of, self.n_groups = list(group_of), int(n_groups)
        self.group = torch.tensor(self.group_of, dtype=torch.int32, device=self.device)
        self.state = torch.zeros(3, self.n_groups, dtype=torch.float64, device=self.device)
        self.scale = torch.ones(self.n_agents, dtype=torch.float64, device=self.device)

    count = property(lambda self: self.state[0])
    mean = property(lambda self: self.state[1])

    @property
    def var(self):
        """The population variance ``m2 / count`` of the returns (0 where nothing has been counted)."""
        return self.state[2] / self.state[0].clamp(min=1.0)

    @property
    def std(self):
        return self.var.sqrt()

    def _window(self, reward, what):
        """``(T, E)`` of a contiguous float32 ``[T,E,N]`` on the normaliser's device."""
        import torch
        if not torch.is_tensor(reward) or reward.dtype != torch.float32 or not reward.is_contiguous() or reward.numel() == 0:
            raise ValueError(f"{what} must be a non-empty contiguous float32 tensor")
        if reward.dim() != 3 or reward.shape[2] != self.n_agents:
            raise ValueError(f"{what} must be [T,E,N] with N = {self.n_agents}, got {tuple(reward.shape)}")
        if not reward.is_cuda or reward.device != self.state.device:
            raise RuntimeError(f"{what} must live on the normaliser's ROCm device {self.state.device} (no CPU fallback)")
        return int(reward.shape[0]), int(reward.shape[1])

    def _workspace(self, T, E):
        import torch
        from . import _native
        if (T, E) not in self._ws_bytes:
            n = self._ws_bytes[(T, E)] = _native.workspace("dronesim_rewnorm_workspace", T, E, self.n_agents)
            if self._ws is None or self._ws.numel() * 8 < n:
                self._ws = torch.empty((n + 7) // 8, dtype=torch.float64, device=self.device)
        return self._ws, self._ws_bytes[(T, E)]

    def update(self, reward, done):
        """Scan the window ``reward [T,E,N]`` (float32) / ``done [T,E]`` (uint8) forward from the carry, merge every finite
        return into its group's moments and rewrite the scale.  The carry is made for the first call's E; another E raises."""
        import torch
        from . import _native
        T, E = self._window(reward, "reward")
        if not (torch.is_tensor(done) and done.dtype == torch.uint8 and done.is_contiguous() and tuple(done.shape) == (T, E)
                and done.device == reward.device):
            raise ValueError(f"done must be a contiguous uint8 tensor of shape {(T, E)} on {reward.device}")
        if self.ret is None:
            self.ret = torch.zeros(E, self.n_agents, dtype=torch.float64, device=self.device)
        elif self.ret.shape[0] != E:
            raise ValueError(f"the carry is for {self.ret.shape[0]} envs, this window has {E} (a normaliser follows one set of envs)")
        ws, ws_bytes = self._workspace(T, E)
        _native.call("dronesim_rewnorm_update", reward, done, T, E, self.n_agents, self.gamma, self.group, self.n_groups, self.ret,
                     self.state, self.scale, self.eps, ws, ws_bytes, device=self.device)
        return self

    def norm(self, reward, out=None):
        """The map with the scale as it stands.  Returns ``out`` (a contiguous float32 tensor of reward's shape; ``out=reward``
        works in place), or an owned buffer that is reused for every later input of this shape."""
        import torch
        from . import _native
        T, E = self._window(reward, "reward")
        if out is None:
            out = self._out.get(tuple(reward.shape))
            if out is None:
                out = self._out[tuple(reward.shape)] = torch.empty_like(reward)
        elif not (torch.is_tensor(out) and out.dtype == torch.float32 and out.is_contiguous() and out.device == reward.device
                  and tuple(out.shape) == tuple(reward.shape)):
            raise ValueError(f"out must be a contiguous float32 tensor of shape {tuple(reward.shape)} on {reward.device}")
        _native.call("dronesim_rewnorm_apply", reward, out, T, E, self.n_agents, self.scale, 0.0 if self.clip is None else self.clip,
                     device=self.device)
        return out

    __call__ = norm

    def reset_carry(self):
        """Zero the running returns, on the device: for a caller who resets the envs by hand between windows (the statistics
        stay)."""
        if self.ret is not None:
            self.ret.zero_()
        return self

    def reset(self):
        """Forget everything: statistics zero, scale 1, carry zero, on the device."""
        self.state.zero_()
        self.scale.fill_(1.0)
        return self.reset_carry()

    def check_agents(self, n_agents):
        """ValueError unless the normaliser is built for ``n_agents`` agents."""
        if int(n_agents) != self.n_agents:
            raise ValueError(f"the reward normaliser is built for {self.n_agents} agents, the networks for {n_agents}")

    def state_dict(self):
        """The statistics as a CPU float64 tensor, with ``gamma``, ``clip``, ``eps`` and the group map (this synchronises the
        host).  The carry is not part of a checkpoint."""
        return dict(state=self.state.detach().cpu().clone(), gamma=self.gamma, clip=self.clip, eps=self.eps,
                    group=list(self.group_of), n_agents=self.n_agents)

    def load_state_dict(self, sd):
        """Take the statistics, ``gamma``, ``clip``, ``eps`` and the group map of `state_dict`'s dict; the scale is rebuilt from
        the state by its definition and the carry is zeroed.  Another number of agents raises ValueError."""
        import torch
        if int(sd["n_agents"]) != self.n_agents:
            raise ValueError(f"the statistics are for {sd['n_agents']} agents, this normaliser for {self.n_agents}")
        group_of, n_groups = _groups(list(sd["group"]), self.n_agents)
        state = torch.as_tensor(sd["state"])
        if tuple(state.shape) != (3, n_groups):
            raise ValueError(f"the statistics have shape {tuple(state.shape)}, their group map {n_groups} groups")
        clip, eps, gamma = _check_clip(sd["clip"]), float(sd["eps"]), float(sd["gamma"])
        if not (eps >= 0 and math.isfinite(eps)):
            raise ValueError(f"eps must be a finite number >= 0, got {eps!r}")
        if not 0.0 <= gamma <= 1.0:
            raise ValueError(f"gamma must be in [0, 1], got {gamma!r}")
        self.clip, self.eps, self.gamma = clip, eps, gamma
        if group_of != self.group_of:
            self._set_groups(group_of, n_groups)
        state = state.to(dtype=torch.float64, device="cpu")
        self.state.copy_(state)
        self.scale.copy_(scale_of_state(state, eps)[torch.tensor(self.group_of, dtype=torch.long)])
        return self.reset_carry()
