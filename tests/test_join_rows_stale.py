"""msj_join_rows_device on arrays that hold a larger join's leftovers (the manner of tests/test_stale_tails.py, whose helpers
are for windows and are not needed here): the SAME context and the SAME caller tensors first take a larger join -- more left
rows, more right rows, more keys, more pairs -- and then, without anything being cleared, a smaller one whose counts are
given on the device only, with poison keys behind L and R.  The workspace holds the larger call's counts, runs, offsets and
ordered rows behind what the smaller one uses, and the outputs hold its pairs behind M: every output is compared over its
WHOLE tensor, the larger join's own entries being what has to remain behind M, pairs_capacity's use and d_offsets[L]."""
import numpy as np
import pytest

from tests import test_join_rows as tjr
from tests import test_join_rows_math as tjm
from tests.test_join_rows import dev, jtw  # noqa: F401

pytestmark = pytest.mark.gpu

BIG_L, BIG_R, BIG_G = 9000, 8000, 70000
SMALL_L, SMALL_R, SMALL_G = 3001, 2049, 300


def big_keys(seed):
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, BIG_G, 2000)
    draw = lambda n: np.where(rng.random(n) < 0.1, -2, rng.choice(pool, n)).astype(np.int32)
    return draw(BIG_L), draw(BIG_R)


@pytest.mark.parametrize("kind", tjm.KINDS)
def test_small_join_over_a_larger_ones_leftovers(dev, jtw, kind):  # noqa: F811
    rng = np.random.default_rng(50 + kind)
    lk, rk = big_keys(kind)
    big = tjm.np_join(lk, rk, BIG_L, BIG_R, BIG_G, kind)
    room = big[3][0] + 100
    held = tjr.Held(dev, lk, rk, room)
    left, right, off, *_ = held.call(BIG_G, kind, keys_capacity=BIG_G)
    M_big = big[3][0]
    assert np.array_equal(left[:M_big], big[0]) and np.array_equal(right[:M_big], big[1]) and np.array_equal(off[:BIG_L + 1], big[2])
    # the smaller join in the same tensors: its keys in front, poison behind L and R (keys that WOULD match, and wild ones)
    import torch

    small_l = np.where(rng.random(SMALL_L) < 0.1, -1, rng.integers(0, SMALL_G, SMALL_L)).astype(np.int32)
    small_r = np.where(rng.random(SMALL_R) < 0.1, SMALL_G, rng.integers(0, SMALL_G, SMALL_R)).astype(np.int32)
    lk2, rk2 = lk.copy(), rk.copy()
    lk2[:SMALL_L], rk2[:SMALL_R] = small_l, small_r
    lk2[SMALL_L:SMALL_L + 500], rk2[SMALL_R:SMALL_R + 500] = 7, 7
    lk2[SMALL_L + 500:SMALL_L + 600], rk2[SMALL_R + 500:SMALL_R + 600] = 0x7FFFFFFF, -0x80000000
    held.d_lk.copy_(torch.from_numpy(lk2).to(dev.device)), held.d_rk.copy_(torch.from_numpy(rk2).to(dev.device))
    left2, right2, off2, res, lsel, rsel = held.call(BIG_G, kind, counts=(SMALL_L, SMALL_R, SMALL_G), keys_capacity=BIG_G)
    small = tjm.np_join(lk2, rk2, SMALL_L, SMALL_R, SMALL_G, kind)
    want = tjm.twin_join(jtw, lk2, rk2, BIG_G, kind, L=SMALL_L, R=SMALL_R, G_dev=SMALL_G, keys_capacity=BIG_G, pairs_capacity=room)
    M = small[3][0]
    assert 0 < M < M_big and want.counters() == small[3]
    assert np.array_equal(res, np.frombuffer(bytes(want.res), dtype=np.uint8))
    assert np.array_equal(lsel, np.frombuffer(bytes(want.lsel), dtype=np.uint8)) and np.array_equal(rsel, lsel)
    # in front of M the smaller join, behind it the larger one's entries and the fill, untouched
    exp_left, exp_right, exp_off = left.copy(), right.copy(), off.copy()
    exp_left[:M], exp_right[:M], exp_off[:SMALL_L + 1] = small[0], small[1], small[2]
    assert np.array_equal(want.left[:M], small[0]) and np.array_equal(want.right[:M], small[1])
    for name, got, exp in (("left rows", left2, exp_left), ("right rows", right2, exp_right), ("offsets", off2, exp_off)):
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (name, int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]), int(bad.size), M)
