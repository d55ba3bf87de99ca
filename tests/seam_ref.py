"""Shared pieces of the policy / learner seam tests (tests/test_gpu_policy_learner_seam.py, tests/test_policy_learner_seam_host.py):
the shapes, the bars and the float64 statements both files use (test infrastructure; CPU or GPU tensors, needs no GPU itself).

The seam: the acting kernels (`BatchedMLP.forward` / `sample_action`) read PACKED snapshots of the weights (`BatchedMLP._packed`), the
learner (csrc/learner.hip) reads and writes the plain arrays ``w1 .. b3`` and re-packs the snapshots once per network per ``train()``."""
import math

import numpy as np
import torch

from tests import learner_ref as R
from tests.sampling_ref import unit_action
from tests.test_gpu_policy_extremes import ROW_BLOCK

N, T, D_IN = 5, 6, 6                                  # agents, steps per window, (k_closest + 1) x c = 3 x 2 observation entries
HIDDEN = (48, 40)                                     # no multiples of 32
T0 = 196                                              # the env's clock before window 1: the time limit (t >= 199) fires in slot 3
GAMMA = 0.99
LR = 1e-3                                             # both learners' default rates, which tests/test_policy_learner_seam_host.py shows to be enough
KINDS = ("softmax", "gaussian")
OUT_KIND = {"critic": 0, "softmax": 1, "gaussian": 2}
TEETH = 10.0                                          # a stale image must miss the bar by this factor at least

# the learner paths of the image test: label -> (learner class, its keywords)
LEARNERS = {"sa2c": ("SA2CLearner", {}),
            "ppo-e3": ("PPOLearner", dict(epochs=3)),
            "ppo-e2-mb3": ("PPOLearner", dict(epochs=2, minibatches=3)),
            "ppo-frozen": ("PPOLearner", dict(epochs=3, target_kl=1e-30)),        # every actor takes exactly one step
            "ppo-guards": ("PPOLearner", dict(epochs=3, target_kl=1e30, vf_clip=0.2))}


def envs_of(config):
    """E of a configuration: its row block + 1, so that a second, ragged workgroup runs."""
    return ROW_BLOCK[config] + 1


def setup_of(config, kind):
    """The keywords of `test_gpu_learner.storage_parts` for one (configuration, actor kind)."""
    return dict(N=N, E=envs_of(config), T=T, t0=T0, config=config, actor_kind=kind, actor_hidden=HIDDEN, critic_hidden=HIDDEN)


def bar_of(config):
    """(rtol, atol factor) of the acting kernels' outputs against float64 (tests/test_gpu_parity.py:
    test_policy_shape_fuzz_all_precisions): |out - ref| <= atol x max(1, max |ref|) + rtol |ref|."""
    return (3e-2, 3e-2) if config == "bf16" else (2e-5, 1e-5)


def out_bar(config):
    """The absolute bar B on an output in [0, 1] (a probability, a variance) or [-1, 1] (a mean): the atol above at max |ref| <= 1."""
    return bar_of(config)[1]


def head(kind, O):
    """Post-activation outputs of the pre-activation ones ``O [..., nout]`` (float64), as `BatchedMLP.forward` returns them."""
    k = OUT_KIND.get(kind, kind)
    if k == 0:
        return O
    if k == 1:
        return torch.softmax(O, -1)
    return torch.cat([torch.tanh(O[..., :2]), torch.sigmoid(O[..., 2:])], -1)


def forward64(W, x, kind):
    """``x [R, N, d]`` -> the float64 outputs ``[R, N, nout]`` of the networks ``W`` (six stacked tensors), head applied."""
    O = R.forward([w.double().cpu() for w in W], x.double().cpu())[2]                 # [N, R, nout]
    return head(kind, O).transpose(0, 1)


def misses(out, ref, config):
    """Per agent, the worst |out - ref| in units of the configuration's bar: <= 1 passes.  out, ref ``[R, N, nout]``."""
    rtol, atol = bar_of(config)
    ref = ref.double().cpu()
    tol = atol * max(1.0, float(ref.abs().max())) + rtol * ref.abs()
    return ((out.double().cpu() - ref).abs() / tol).amax(dim=(0, 2))


def gaussian_logp(a, out):
    """The float64 log-density of the actions ``a [..., 2]`` at ``out = (mu_x, mu_y, var_x, var_y) [..., 4]``, and the first-order
    sensitivity ``sum_d |a - mu| / var + (a - mu)^2 / (2 var^2) + 1 / (2 var)`` of it to an error of the four outputs."""
    a, out = a.double(), out.double()
    mu, var = out[..., :2], out[..., 2:]
    d = a - mu
    lp = (-0.5 * torch.log(2 * math.pi * var) - d * d / (2 * var)).sum(-1)
    sens = (d.abs() / var + d * d / (2 * var * var) + 1 / (2 * var)).sum(-1)
    return lp, sens


def gaussian_region(out):
    """The rows of ``out [..., 4]`` inside the compared region: every variance in [0.05, 0.95], every |mean| <= 0.98."""
    out = out.double()
    return ((out[..., 2:] >= 0.05) & (out[..., 2:] <= 0.95)).all(-1) & (out[..., :2].abs() <= 0.98).all(-1)


def unit_vectors32(nout):
    """The ideal float32 unit vectors ``[nout, 2]`` of the action list: (cos, sin)(2 pi j / nout) rounded from float64."""
    return unit_action(np.arange(nout), nout).astype(np.float32)


def step_ulps(v, k):
    """The float32 array ``v`` moved by ``k`` units in the last place (``k`` an integer array of v's shape)."""
    v, k = np.array(v, np.float32), np.broadcast_to(np.asarray(k), np.shape(v))
    for _ in range(int(np.abs(k).max(initial=0))):
        todo = k != 0
        v = np.where(todo, np.nextafter(v, np.where(k > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)), v)
        k = k - np.sign(k) * todo
    return v.astype(np.float32)


def synthetic_window(kind, E, seed=11, obs_scale=3.0):
    """A window of the GPU tests' shape for the host tests (CPU tensors): observations uniform in [-obs_scale, obs_scale] (the env's
    are differences of positions in a 10 x 10 box, of that order), rewards ~ -|N(0, 1)| x 5, one episode end in slot 3 of every env,
    actions on the action list (softmax) or N(0, 0.7) (Gaussian), neighbour lists with the self entry first and a ghost slot."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(T, E, N, D_IN, generator=g) * 2 - 1) * obs_scale
    reward = -(torch.randn(T, E, N, generator=g).abs() * 5)
    done = torch.zeros(T, E, dtype=torch.uint8)
    done[199 - T0] = 1
    if kind == "softmax":
        a = torch.randint(0, 16, (T, E, N), generator=g).double() * 2 * math.pi / 16
        act = torch.stack([a.cos(), a.sin()], -1).float()
    else:
        act = torch.randn(T, E, N, 2, generator=g) * 0.7
    nbr = torch.stack([torch.arange(N)[None, None, :].expand(T, E, N), torch.randint(0, N, (T, E, N), generator=g),
                       torch.randint(-1, N, (T, E, N), generator=g)], -1).int()
    return x, reward, done, act, nbr
