"""Host restatement of `BatchedMLP.sample_action`'s sampling tail (csrc/policy_common.hpp: finish_quad), numpy / float64,
no GPU (test infrastructure).

The contract it states ("Policy sampling: the stream and the pick"):

  stream     philox4x32-10(ctr = (agent, env_base + e, counter.lo + t[e], counter.hi + episode[e]); key = (seed.lo, seed.hi)),
             every counter word modulo 2^32 on its own (no carry from word 2 into word 3)
  pick       u = (word 0 >> 8) / 2^24; the FIRST j with u < cdf_j, cdf = running sum of the probabilities; nout - 1 if there is none
  action     (cos, sin)(2 pi pick / nout)
  Gaussian   component d uses words (2 d, 2 d + 1): u1 = ((w >> 8) + 1) / 2^24, u2 = (w' >> 8) / 2^24,
             act_d = mu_d + sqrt(var_d) * sqrt(-2 ln u1) * cos(2 pi u2)

The Philox below is a second implementation on purpose (tests/test_sampling_host.py pins it against the oracle's, which is pinned on the
Random123 known answers).  `categorical_pick` does NOT mirror the kernel's summation order: it sums the kernel's own float32
probabilities in float64 and marks as `ambiguous` every draw that sits within delta = nout * 2^-23 of a cdf value -- the kernel adds at
most nout float32 terms <= 1 in an order of its own, each addition rounding by at most 2^-24; the factor 2 is margin.

The second half of the file generates the networks and inputs of tests/test_gpu_sampling.py, so that the host test
(tests/test_sampling_host.py) can check the band's share on the very same cases without a GPU."""
import zlib

import numpy as np

M32 = 0xFFFFFFFF


def _u32(a):
    return np.asarray(a, dtype=np.uint64) & np.uint64(M32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11), vectorised over uint32 arrays (broadcast against each other) -> four uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[_u32(v) for v in (c0, c1, c2, c3, k0, k1)])
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    mask, sh = np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & mask, (p0 >> sh) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + w0) & mask, (k1 + w1) & mask
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def draw_words(seed, counter, env_base, E, N, t=None, episode=None):
    """The four words every (env row e, agent) of one `sample_action` call draws: uint32 [E, N, 4].
    `seed`, `counter` 64-bit, `env_base` the global id of row 0, `t` / `episode` the env's int32 [E] counters (None = 0)."""
    seed, counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    e = np.arange(E, dtype=np.int64)
    tt = np.zeros(E, np.int64) if t is None else np.asarray(t, np.int64).reshape(E)
    ep = np.zeros(E, np.int64) if episode is None else np.asarray(episode, np.int64).reshape(E)
    c1 = np.array([(int(env_base) + int(i)) & M32 for i in e], dtype=np.uint64)
    c2 = ((counter & M32) + tt) & M32                      # word by word: no carry into the high word
    c3 = ((counter >> 32) + ep) & M32
    agent = np.arange(N, dtype=np.uint64)
    w = philox4x32_10(agent[None, :], c1[:, None], c2[:, None], c3[:, None], seed & M32, seed >> 32)
    return np.stack(w, axis=-1)


def uniform24(w):
    """(w >> 8) / 2^24 in [0, 1): exact in float32 and in float64."""
    return (np.asarray(w, np.uint32) >> np.uint32(8)).astype(np.float64) / 16777216.0


def categorical_pick(p, words):
    """p [..., nout] (the kernel's own float32 probabilities), words [..., 4] -> (pick, ambiguous, u)."""
    p = np.asarray(p)
    nout = p.shape[-1]
    u = uniform24(np.asarray(words)[..., 0])
    cdf = np.cumsum(p.astype(np.float64), axis=-1)
    pick = np.minimum((~(u[..., None] < cdf)).sum(-1), nout - 1)
    delta = nout * 2.0 ** -23
    ambiguous = (np.abs(u[..., None] - cdf) <= delta).any(-1)
    return pick, ambiguous, u


def unit_action(idx, nout):
    a = 2.0 * np.pi * np.asarray(idx, np.float64) / nout
    return np.stack([np.cos(a), np.sin(a)], axis=-1)


def gaussian_action(mu, var, words):
    """mu, var [..., 2], words [..., 4] -> (act [..., 2], r [..., 2]), r = the Box-Muller radius sqrt(-2 ln u1)."""
    words = np.asarray(words)
    u1 = ((words[..., 0::2] >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = uniform24(words[..., 1::2])
    r = np.sqrt(-2.0 * np.log(u1))
    act = np.asarray(mu, np.float64) + np.sqrt(np.asarray(var, np.float64)) * r * np.cos(2.0 * np.pi * u2)
    return act, r


# ------------------------------------------------------------------ the cases of tests/test_gpu_sampling.py
NOUTS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32)              # every `valid` pattern of the last group of four, every count of groups
SHAPES = ((1, 1), (3, 65), (5, 130), (9, 257))             # (N, E): work lists that do not divide by 8, ragged last tiles, > 1 tile per agent
WIDE = (64, 70)                                            # at nout = 16 (and the Gaussian): the `div_magic` path with many agents
CLASSES = ("ordinary", "peaked", "uniform")
CAP = 1e-3                                                 # largest share of a case's draws that may sit in the band

# Where a draw of a case sat inside the band at a shape too small to absorb it (one draw in 650 is above the cap), the
# case's inputs were re-drawn with the next salt (keyed by the case's tag): the cap is a condition on the inputs, and it stays.
SALTS = {"softmax ordinary nout=32 N=5 E=130 d=6 h1=33 h2=65": 2,       # (plain bf16's own probabilities: 2 of 650; salt 1: host 1 of 650)
         "softmax uniform nout=32 N=5 E=130 d=6 h1=33 h2=65": 1,        # (host: 1 of 650 draws in the band at salt 0)
         "softmax uniform nout=31 N=3 E=65 d=15 h1=33 h2=65": 1,        # (host: 1 of 195)
         "softmax uniform nout=9 N=5 E=130 d=6 h1=33 h2=129": 1}        # (host: 1 of 650)


def grid_cases():
    """(nout, N, E) of the fixed grid."""
    out = [(nout, N, E) for nout in NOUTS for (N, E) in SHAPES]
    out.append((16,) + WIDE)
    return out


def _rng(tag, salt):
    return np.random.default_rng([zlib.crc32(tag.encode()), salt])


def _network(rng, N, d, h1, h2, nout, sc3=1.2):
    u = lambda *s: rng.uniform(-1.0, 1.0, s).astype(np.float32)
    return [u(N, d, h1) * np.float32(0.8 / np.sqrt(d)), u(N, h1) * np.float32(0.3), u(N, h1, h2) * np.float32(1.2 / np.sqrt(h1)),
            u(N, h2) * np.float32(0.3), u(N, h2, nout) * np.float32(sc3 / np.sqrt(h2)), u(N, nout) * np.float32(0.3)]


def softmax_case(cls, nout, N, E, d=6, h1=33, h2=65):
    """One categorical case: dict(w = [w1, b1, w2, b2, w3, b3] float32, x [E, N, d] float32, seed, counter, env_base, tag).
    `cls`: "ordinary"; "peaked" = w3, b3 * 40 (tails underflow to probability exactly 0); "uniform" = w3 = b3 = 0."""
    tag = f"softmax {cls} nout={nout} N={N} E={E} d={d} h1={h1} h2={h2}"
    rng = _rng(tag, SALTS.get(tag, 0))
    w = _network(rng, N, d, h1, h2, nout, sc3=4.0)
    if cls == "peaked":
        w[4], w[5] = w[4] * np.float32(40.0), w[5] * np.float32(40.0)
    elif cls == "uniform":
        w[4], w[5] = np.zeros_like(w[4]), np.zeros_like(w[5])
    elif cls != "ordinary":
        raise ValueError(cls)
    x = rng.uniform(-3.0, 3.0, (E, N, d)).astype(np.float32)
    return dict(w=w, x=x, seed=int(rng.integers(0, 2 ** 63)), counter=int(rng.integers(0, 2 ** 63)),
                env_base=int(rng.integers(0, 2 ** 40)), tag=tag)


def gaussian_case(N, E, d=6, h1=33, h2=65):
    """One Gaussian case (out_kind 2, nout = 4, block-diagonal w3: the first half of layer 2 feeds the means, the second the variances)."""
    tag = f"gaussian N={N} E={E} d={d} h1={h1} h2={h2}"
    rng = _rng(tag, 0)
    w = _network(rng, N, d, h1, h2, 4, sc3=6.0)
    half = h2 // 2
    w[4][:, :half, 2:] = 0.0
    w[4][:, half:, :2] = 0.0
    x = rng.uniform(-3.0, 3.0, (E, N, d)).astype(np.float32)
    return dict(w=w, x=x, seed=int(rng.integers(0, 2 ** 63)), counter=int(rng.integers(0, 2 ** 63)),
                env_base=int(rng.integers(0, 2 ** 40)), tag=tag)


def host_logits(w, x):
    """The three layers in float64: [E, N, nout] pre-activation outputs."""
    w1, b1, w2, b2, w3, b3 = [np.asarray(a, np.float64) for a in w]
    h = np.maximum(np.einsum("end,ndh->enh", np.asarray(x, np.float64), w1) + b1, 0.0)
    h = np.maximum(np.einsum("enh,nhk->enk", h, w2) + b2, 0.0)
    return np.einsum("enk,nko->eno", h, w3) + b3


def host_softmax(w, x):
    y = host_logits(w, x)
    y = np.exp(y - y.max(-1, keepdims=True))
    return y / y.sum(-1, keepdims=True)
