"""msj_dictionary_order_device on arrays that hold a larger dictionary's leftovers (the manner of
tests/test_join_rows_stale.py): the SAME context and the SAME caller tensors first order a larger dictionary and then,
without anything being cleared, a smaller one whose V is given on the device only, with live-looking offsets behind V --
entries that would pass the entry test.  The workspace holds the larger call's keys, places and counts behind what the
smaller one uses, d_sorted / d_rank hold its entries behind V: every output is compared over its WHOLE tensor, the larger
call's own entries being what has to remain behind V."""
import numpy as np
import pytest

from tests import test_dictionary_order as tdo
from tests import test_dictionary_order_math as tdm
from tests.test_dictionary_order import dev, tw  # noqa: F401

pytestmark = pytest.mark.gpu


def values(seed, n):
    import random

    rng = random.Random(seed)
    shared = tdm.word(rng, 10)
    return [None if rng.random() < 0.03 else shared + tdm.word(rng, rng.choice((0, 1, 4, 8, 9, 14))) for _ in range(n)]


@pytest.mark.parametrize("big_v,small_v,mode", ((3000, 1100, tdm.GRID), (1024, 300, tdm.GROUP), (1024, 300, tdm.GRID)))
def test_small_dictionary_over_a_larger_ones_leftovers(dev, tw, big_v, small_v, mode):  # noqa: F811
    import torch

    big = tdm.Dict(values(1, big_v))
    held = tdo.Held(dev, big)
    rc, (srt, rnk, _) = held.call(mode, max_rounds=64)
    _, want_big, ws_big, wr_big, _ = tdm.run_twin(tw, big, max_rounds=64, mode=mode)
    assert rc == 0 and np.array_equal(srt[:big_v], ws_big) and np.array_equal(rnk[:big_v], wr_big) and want_big.code == 0
    # the smaller dictionary in the same tensors: its offsets in front, entries that look alive behind V, its bytes over the others'
    small = tdm.Dict(values(2, small_v), extra=big_v - small_v)
    assert small.cap <= big.cap and small.offsets.size == big.offsets.size
    held.d_offsets.copy_(tdo.to_dev(dev, small.offsets))
    held.raw[:small.cap] = torch.from_numpy(small.bytes.copy()).to(dev.device)
    held.bytes_ptr, held.d = held.raw.data_ptr(), small
    d_n = torch.tensor([small_v], dtype=torch.int64, device=dev.device)
    rc, (srt2, rnk2, res2) = held.call(mode, max_rounds=64, d_n_entries=d_n.data_ptr(), n_entries=big_v)
    rc2, want, ws, wr, _ = tdm.run_twin(tw, small, capacity=big_v, max_rounds=64, mode=mode, on_device=True)
    assert rc == 0 and rc2 == 0 and want.code == 0 and 0 < want.n_values < small_v
    tdm.check_against(small.values, want, ws, wr, None, big_v)
    assert res2 == bytes(want), (tdo.fields(res2), tdo.fields(bytes(want)))
    exp_s, exp_r = srt.copy(), rnk.copy()
    exp_s[:small_v], exp_r[:small_v] = ws[:small_v], wr[:small_v]
    for name, got, exp in (("sorted", srt2, exp_s), ("rank", rnk2, exp_r)):
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (name, int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]), int(bad.size))
