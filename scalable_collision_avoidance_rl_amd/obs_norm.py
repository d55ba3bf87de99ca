"""Observation normalisation: running per-(agent, input column) mean and variance, kept and applied on the device.

The networks of a `BatchedMLP` read ``z`` rows in grid units: at G = 5 they are O(1), at G = 28 or 256 an agent's goal offset is
tens to hundreds of units next to neighbour offsets of O(Delta).  `ObsNormalizer` keeps, per agent and input column, the count,
mean and sum of squared deviations of every finite value it has been shown (csrc/obsnorm.hip: float64, Chan's merge, one fixed
reduction order) and maps observations with the table made from them:

    norm = ObsNormalizer(env.n_agents, env.local_state_space, env.device)
    actor.sample_action(norm(env.z), env=env, act_out=storage.actions[t])       # the rollout loop
    learner = PPOLearner(actor, critic, gamma, obs_norm=norm)                   # train() normalises the window, then updates

  update(x)   dronesim_obsnorm_update   merge the finite values of ``x [..., N, d]`` (any leading dims are rows) into the state and
                                        rewrite the table
  norm(x)     dronesim_obsnorm_apply    ``(x - mean) / sqrt(var + eps)``, clamped to ``[-clip, clip]``; NaN stays NaN

Both enqueue kernels only -- no host synchronisation, no memset node, nothing allocated after the first call per shape -- so a
rollout window, ``train()`` and the update replay from one captured graph.  Importing this module needs neither a GPU nor the built
library; `update` and `norm` need both (no CPU fallback).  A normaliser on the CPU only carries statistics (`state_dict`)."""
from __future__ import annotations

import math


def _check_clip(clip):
    """None (no clamp) or a finite number > 0, else ValueError."""
    import numbers
    if clip is None:
        return None
    if isinstance(clip, bool) or not isinstance(clip, numbers.Real) or not math.isfinite(clip) or clip <= 0:
        raise ValueError(f"clip must be None or a finite number > 0, got {clip!r}")
    return float(clip)


class ObsNormalizer:
    """Running statistics of ``N x d`` observation columns.  ``state [3,N,d]`` = (count, mean, m2) and ``table [2,N,d]`` =
    (mean, 1 / sqrt(m2 / count + eps)) are float64 tensors on ``device`` that only the kernels write; a fresh normaliser
    (count 0) holds the identity table.  ``clip=None``: no clamp."""

    def __init__(self, n_agents, d_in, device, clip=10.0, eps=1e-8):
        import numbers
        import torch
        if int(n_agents) != n_agents or int(d_in) != d_in or n_agents < 1 or d_in < 1:
            raise ValueError(f"n_agents and d_in must be integers >= 1, got {n_agents!r} and {d_in!r}")
        if isinstance(eps, bool) or not isinstance(eps, numbers.Real) or not math.isfinite(eps) or eps < 0:
            raise ValueError(f"eps must be a finite number >= 0, got {eps!r}")
        self.n_agents, self.d_in, self.device = int(n_agents), int(d_in), torch.device(device)
        self.clip, self.eps = _check_clip(clip), float(eps)
        self.C = self.n_agents * self.d_in
        self.state = torch.zeros(3, self.n_agents, self.d_in, dtype=torch.float64, device=self.device)
        self.table = torch.zeros(2, self.n_agents, self.d_in, dtype=torch.float64, device=self.device)
        self.table[1].fill_(1.0)
        self._ws = None
        self._ws_bytes = {}                 # rows -> workspace bytes of that row count
        self._out = {}                      # input shape -> the owned output buffer of `norm`

    count = property(lambda self: self.state[0])
    mean = property(lambda self: self.state[1])

    @property
    def var(self):
        """The population variance ``m2 / count`` (0 where nothing has been counted)."""
        return self.state[2] / self.state[0].clamp(min=1.0)

    def _rows(self, x, what):
        """Rows of ``x`` as an ``[R][N d]`` matrix; checks dtype, layout, device and that trailing dims flatten to ``N d``."""
        import torch
        if not torch.is_tensor(x) or x.dtype != torch.float32 or not x.is_contiguous() or x.numel() == 0:
            raise ValueError(f"{what} must be a non-empty contiguous float32 tensor")
        if not x.is_cuda or x.device != self.state.device:
            raise RuntimeError(f"{what} must live on the normaliser's ROCm device {self.state.device} (no CPU fallback)")
        tail = 1
        for n in reversed(x.shape):
            tail *= n
            if tail >= self.C:
                break
        if tail != self.C:
            raise ValueError(f"the trailing dims of {what} {tuple(x.shape)} do not flatten to N d = {self.n_agents} x {self.d_in}")
        return x.numel() // self.C

    def _workspace(self, R):
        import torch
        from . import _native
        if R not in self._ws_bytes:
            n = self._ws_bytes[R] = _native.workspace("dronesim_obsnorm_workspace", R, self.C)
            if self._ws is None or self._ws.numel() * 8 < n:
                self._ws = torch.empty((n + 7) // 8, dtype=torch.float64, device=self.device)
        return self._ws, self._ws_bytes[R]

    def update(self, x):
        """Merge the finite values of ``x`` (``[T,E,N,d]``, ``[E,N,k+1,c]``, ... : leading dims are rows) into the statistics and
        rewrite the table."""
        from . import _native
        R = self._rows(x, "x")
        ws, ws_bytes = self._workspace(R)
        _native.call("dronesim_obsnorm_update", x, R, self.C, self.state, self.table, self.eps, ws, ws_bytes, device=self.device)
        return self

    def norm(self, x, out=None):
        """The map with the table as it stands.  Returns ``out`` (a contiguous float32 tensor of x's shape; ``out=x`` works in
        place), or an owned buffer that is reused for every later input of this shape."""
        import torch
        from . import _native
        R = self._rows(x, "x")
        if out is None:
            out = self._out.get(tuple(x.shape))
            if out is None:
                out = self._out[tuple(x.shape)] = torch.empty_like(x)
        elif not (torch.is_tensor(out) and out.dtype == torch.float32 and out.is_contiguous() and out.device == x.device
                  and tuple(out.shape) == tuple(x.shape)):
            raise ValueError(f"out must be a contiguous float32 tensor of shape {tuple(x.shape)} on {x.device}")
        _native.call("dronesim_obsnorm_apply", x, out, R, self.C, self.table, 0.0 if self.clip is None else self.clip, device=self.device)
        return out

    __call__ = norm

    def reset(self):
        """Forget everything: the state becomes zero and the table the identity, on the device."""
        self.state.zero_()
        self.table[0].zero_()
        self.table[1].fill_(1.0)
        return self

    def check_networks(self, *nets):
        """ValueError unless every network reads ``N`` agents x ``d`` inputs."""
        for net in nets:
            if net is not None and (net.n_agents, net.d_in) != (self.n_agents, self.d_in):
                raise ValueError(f"the normaliser is built for {self.n_agents} agents x {self.d_in} inputs, the network for "
                                 f"{net.n_agents} x {net.d_in}")

    def state_dict(self):
        """The statistics as CPU float64 tensors, with ``clip``, ``eps`` and the shape (this synchronises the host)."""
        return dict(state=self.state.detach().cpu().clone(), clip=self.clip, eps=self.eps, n_agents=self.n_agents, d_in=self.d_in)

    def load_state_dict(self, sd):
        """Take the statistics, ``clip`` and ``eps`` of `state_dict`'s dict; the table is rebuilt from the state by its
        definition.  A shape that is not this normaliser's raises ValueError."""
        import torch
        state = torch.as_tensor(sd["state"])
        if (int(sd["n_agents"]), int(sd["d_in"])) != (self.n_agents, self.d_in) or tuple(state.shape) != (3, self.n_agents, self.d_in):
            raise ValueError(f"the statistics are for {sd['n_agents']} agents x {sd['d_in']} inputs (state {tuple(state.shape)}), "
                             f"this normaliser for {self.n_agents} x {self.d_in}")
        clip, eps = _check_clip(sd["clip"]), float(sd["eps"])
        if not eps >= 0:
            raise ValueError(f"eps must be >= 0, got {eps!r}")
        self.clip, self.eps = clip, eps
        state = state.to(dtype=torch.float64, device="cpu")
        self.state.copy_(state)
        self.table.copy_(table_of_state(state, eps))
        return self


def table_of_state(state, eps):
    """``table [2,N,d]`` of a ``state [3,N,d]`` (float64, host side): ``(mean, 1 / sqrt(m2 / count + eps))``, 0 where that
    denominator is 0, and ``(0, 1)`` where the count is 0."""
    import torch
    n, mean, m2 = state[0], state[1], state[2]
    seen = n > 0
    var = torch.where(seen, m2 / n.clamp(min=1.0) + eps, torch.ones_like(n))
    inv = torch.where(var > 0, 1.0 / torch.sqrt(var), torch.zeros_like(var))
    return torch.stack([torch.where(seen, mean, torch.zeros_like(mean)), torch.where(seen, inv, torch.ones_like(inv))])
