"""Host-side tests of the shuffled minibatches (no GPU needed): the restated row permutation (tests/minibatch_ref.py) is a
bijection and moves with its counter and seed; the two new entry points are exported with the declared argtypes and decide every
EINVAL case on the host; `PPOLearner`'s new arguments; the minibatch restatement collapses to `ppo_ref.ppo_train` at K = 1."""
import ctypes as C

import numpy as np
import pytest
import torch

from scalable_collision_avoidance_rl_amd import _native
from tests import learner_ref as R
from tests import minibatch_ref as MB
from tests import ppo_ref as P
from tests import test_gpu_learner as TG
from tests.test_ppo_host import host_mlp

R_LIST = (1, 2, 3, 4, 5, 63, 64, 65, 1000, 4097)
MB_SYMBOLS = ("dronesim_row_permutation", "dronesim_gather_rows")


@pytest.mark.parametrize("rows", R_LIST)
def test_restated_permutation_is_a_bijection(rows):
    for seed, counter in ((0, 0), (12345, 1), (2 ** 40 + 3, 7)):
        perm = MB.row_permutation(rows, seed, counter)
        assert perm.shape == (rows,) and np.array_equal(np.sort(perm), np.arange(rows)), (seed, counter)
    assert MB.half_bits(rows) == {1: 1, 2: 1, 3: 1, 4: 1, 5: 2, 63: 3, 64: 3, 65: 4, 1000: 5, 4097: 7}[rows]
    if rows <= 65:                                   # the side-by-side walk is the one-integer-at-a-time rule
        assert np.array_equal(MB.row_permutation(rows, 2 ** 40 + 3, 7), MB.row_permutation_scalar(rows, 2 ** 40 + 3, 7))


def test_restated_permutation_rule_at_its_edges():
    assert MB.half_bits(2 ** 31 - 1) == 16           # the domain is then 2^32
    # the network is a bijection of its whole domain [0, 2^(2h))
    for h in (1, 2, 3):
        assert sorted(MB.feistel(v, h, 99, 5) for v in range(1 << (2 * h))) == list(range(1 << (2 * h)))
    # only the low 32 bits of the counter enter
    assert np.array_equal(MB.row_permutation(100, 3, 9), MB.row_permutation(100, 3, 9 + 2 ** 32))


def test_two_counters_or_two_seeds_give_different_permutations():
    base = MB.row_permutation(1000, 11, 0)
    for seed, counter in ((11, 1), (11, 7), (12, 0), (11 + 2 ** 32, 0)):
        other = MB.row_permutation(1000, seed, counter)
        assert (other != base).mean() > 0.9, (seed, counter)
    assert (base != np.arange(1000)).mean() > 0.9


def test_library_exports_the_minibatch_entry_points_with_the_declared_argtypes():
    lib = _native.lib()
    want = ("dronesim_row_permutation", "dronesim_gather_rows")
    assert set(want) == set(MB_SYMBOLS)
    header = open(_native.HEADER_PATH).read()
    for name in want:
        assert name in _native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int, name
        assert f"int {name}(" in header, name
    assert lib.dronesim_version() == 600


def gather_call(lib, perm=4096, R_=192, M=64, n=2, src=(4096, 8192), dst=(65536, 131072), row_bytes=(72, 12), block_bytes=None,
                null=None):
    """`dronesim_gather_rows` with made-up device addresses (never dereferenced: validation happens on the host)."""
    k = max(len(src), 1)
    block_bytes = tuple(-(-M * rb // 256) * 256 for rb in row_bytes) if block_bytes is None else block_bytes
    args = dict(src=(C.c_void_p * k)(*src), dst=(C.c_void_p * k)(*dst), row_bytes=(C.c_int64 * k)(*row_bytes),
                block_bytes=(C.c_int64 * k)(*block_bytes))
    if null:
        args[null] = None
    return lib.dronesim_gather_rows(perm, R_, M, n, args["src"], args["dst"], args["row_bytes"], args["block_bytes"], None)


def test_minibatch_entry_points_reject_bad_arguments_on_the_host():
    """Every EINVAL case is decided before anything is enqueued (no HIP call: this runs without a GPU)."""
    lib = _native.lib()
    for bad in ((0, 0, 4096, 4096), (-5, 0, 4096, 4096), (10, 0, None, 4096), (10, 0, 4096, None)):
        assert lib.dronesim_row_permutation(*bad, None) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(b"dronesim_row_permutation"), bad
    for bad in (dict(perm=None), dict(null="src"), dict(null="dst"), dict(null="row_bytes"), dict(null="block_bytes"),
                dict(R_=0), dict(R_=-192), dict(M=0), dict(M=-1), dict(M=100),                      # 192 % 100 != 0
                dict(n=0), dict(n=-1), dict(n=9),
                dict(row_bytes=(72, 0)), dict(row_bytes=(72, -4)), dict(row_bytes=(70, 12)), dict(row_bytes=(72, 13)),
                dict(block_bytes=(64 * 72 - 4, 768)), dict(block_bytes=(4608, 0)),                  # a short block
                dict(src=(4096, None)), dict(dst=(None, 131072)), dict(src=(0, 8192)),
                dict(row_bytes=((1 << 24) + 4, 12)),                                                # above DRONESIM_GATHER_MAX_ROW_BYTES
                dict(src=(4098, 8192)), dict(dst=(65536, 131073)), dict(block_bytes=(4610, 768))):  # not multiples of 4
        assert gather_call(lib, **bad) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(b"dronesim_gather_rows"), bad
    nine = dict(n=9, src=(4096,) * 9, dst=(65536,) * 9, row_bytes=(4,) * 9)
    assert gather_call(lib, **nine) == _native.EINVAL


def test_ppo_learner_rejects_bad_minibatches_and_shuffle_seed():
    from types import SimpleNamespace
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    actor, critic = host_mlp(1, 16), host_mlp(0, 1)
    learner = PPOLearner(actor, critic, 0.99)
    assert (learner.minibatches, learner.shuffle_seed) == (1, 0)
    learner = PPOLearner(actor, critic, 0.99, minibatches=8, shuffle_seed=2 ** 64 - 1)
    assert (learner.minibatches, learner.shuffle_seed) == (8, 2 ** 64 - 1)
    assert PPOLearner(actor, critic, 0.99, minibatches=np.int64(4)).minibatches == 4
    for kw in (dict(minibatches=0), dict(minibatches=-2), dict(minibatches=2.0), dict(minibatches=1.5), dict(minibatches=None),
               dict(minibatches="4"), dict(minibatches=True), dict(shuffle_seed=-1), dict(shuffle_seed=2 ** 64),
               dict(shuffle_seed=1.0), dict(shuffle_seed=None), dict(shuffle_seed=False)):
        with pytest.raises(ValueError):
            PPOLearner(actor, critic, 0.99, **kw)
    # T E = 8 rows do not cut into 3 minibatches: refused at _prepare, before any buffer is made
    st = SimpleNamespace(z_pre=torch.zeros(4, 2, 3, 6), reward=torch.zeros(4, 2, 3), done=torch.zeros(4, 2, dtype=torch.uint8),
                         actions=torch.zeros(4, 2, 3, 2), nbr_pre=torch.zeros(4, 2, 3, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="minibatches"):
        PPOLearner(actor, critic, 0.99, minibatches=3).train(st)


def test_gathered_rows_blocks_are_padded_to_256_bytes():
    from scalable_collision_avoidance_rl_amd.learner import MINIBATCH_ALIGN, GatheredRows
    g = GatheredRows((3, 6), 4, 5, "cpu")                        # 5 rows of 72 bytes = 360 -> 512 per block
    assert (g.row_bytes, g.block_bytes, MINIBATCH_ALIGN) == (72, 512, 256) and g.buf.numel() == 4 * 128
    assert [b.shape for b in g.blocks] == [(5, 3, 6)] * 4 and all(b.is_contiguous() for b in g.blocks)
    assert [b.data_ptr() - g.buf.data_ptr() for b in g.blocks] == [0, 512, 1024, 1536]


def test_minibatch_restatement_with_one_block_and_the_identity_is_ppo_train():
    N, E, T, d_in = 3, 4, 9, 6
    gen = torch.Generator().manual_seed(3)
    for kind, nout in ((1, 16), (2, 4)):
        Wa, Wc = TG.random_net(torch, gen, N, d_in, 12, 10, nout), TG.random_net(torch, gen, N, d_in, 9, 11, 1)
        if kind == 2:
            Wa[4] = Wa[4] * R.structural_mask(2, Wa)
        x, _, act, _ = TG.random_rows(torch, gen, T, E, N, d_in, nout, kind)
        reward = torch.randn(T, E, N, generator=gen)
        done = torch.zeros(T, E, dtype=torch.uint8)
        done[4, ::2] = 1
        nbr = torch.stack([torch.arange(N)[None, None, :].expand(T, E, N), torch.randint(-1, N, (T, E, N), generator=gen)], -1).int()
        a = P.ppo_train(kind, Wa, Wc, x, reward, done, act, nbr, 0.97, epochs=3)
        b = MB.ppo_train_minibatch(kind, Wa, Wc, x, reward, done, act, nbr, 0.97, minibatches=1, epochs=3,
                                   perms=[np.arange(T * E)] * 3)
        close = lambda p, q: torch.allclose(p, q, rtol=1e-12, atol=1e-14)
        for ep in range(3):
            assert close(a["critic_loss"][ep], b["critic_loss"][ep][0]) and close(a["actor_loss"][ep], b["actor_loss"][ep][0])
            assert close(a["critic_norm"][ep], b["critic_norm"][ep][0]) and close(a["actor_norm"][ep], b["actor_norm"][ep][0])
            assert torch.equal(a["actor"][ep]["clipped"], b["actor"][ep][0]["clipped"])
        for p, q in zip(a["critic_post"] + a["actor_post"], b["critic_post"] + b["actor_post"]):
            assert close(p, q)
        assert a["state"]["step"] == b["state"]["step"] == 3
        # with K = 3 the step count advances per block, and a shuffled epoch is another update
        c = MB.ppo_train_minibatch(kind, Wa, Wc, x, reward, done, act, nbr, 0.97, minibatches=3, shuffle_seed=5, epochs=2)
        assert c["state"]["step"] == 6 and [len(e) for e in c["critic_loss"]] == [3, 3]
        assert np.array_equal(c["perms"][0], MB.row_permutation(T * E, 5, 0)) and np.array_equal(c["perms"][1], MB.row_permutation(T * E, 5, 3))
        assert not close(c["critic_post"][0], a["critic_post"][0])
