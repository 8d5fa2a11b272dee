"""msj_match_strings_device on arrays that hold a larger column's leftovers (the manner of
tests/test_dictionary_order_stale.py): the SAME context and the SAME caller tensors first match a larger column and then,
without anything being cleared, a smaller one whose R is given on the device only -- with live-looking offsets behind R that
would fail the row test if they were looked at, and the larger column's bytes, pattern included, behind bytes_len.  The
workspace holds the larger call's words and cursors behind what the smaller one uses, the records its rows behind R: every
output is compared over its WHOLE tensor, the larger call's own records being what has to remain behind R."""
import random

import numpy as np
import pytest

from tests import test_match_strings as tms
from tests import test_match_strings_math as tmm
from tests.test_match_strings import dev, tw  # noqa: F401

pytestmark = pytest.mark.gpu


def rows_of(seed, n):
    rng = random.Random(seed)
    return [None if rng.random() < 0.05 else tmm.word(rng, rng.choice((0, 3, 9, 30, 70)), tmm.ALPHABET[1:4]) for _ in range(n)]


def test_small_column_over_a_larger_ones_leftovers(dev, tw):  # noqa: F811
    import torch

    big_r, small_r = 3000, 700
    specs = [b"ab", ([b"a", b"b", b"a"], 0), ([b"ba"], tmm.AT_END), ([b"AB", b"A"], tmm.NOCASE | tmm.AT_START)]
    big = tmm.Column(rows_of(1, big_r))
    held = tms.Held(dev, big, len(specs))
    patterns = dev.compile_patterns(tms.wrapper_specs(specs))
    rc, (fields_big, res_big, _) = held.call(patterns)
    _, want_res, _, want_rec = tmm.run_twin(tw, big, specs)
    assert rc == 0 and res_big == bytes(want_res) and fields_big == tms.with_canary(want_rec, len(specs), big_r)
    # the smaller column in the same tensors: its offsets in front, offsets that break the row test behind R, its bytes over the others'
    small = tmm.Column(rows_of(2, small_r), extra=big_r - small_r)
    assert small.bytes_len < big.bytes_len // 2 and small.offsets.size == big.offsets.size
    small.offsets[small_r + 1:] = big.offsets[small_r + 1:][::-1]   # descending, and past the smaller bytes_len
    held.d_offsets.copy_(torch.from_numpy(small.offsets.view(np.int64).copy()).to(dev.device))
    held.d_valid.fill_(1)
    held.d_valid[:small_r] = torch.from_numpy(small.valid[:small_r].copy()).to(dev.device)
    held.raw[:small.bytes_len] = torch.from_numpy(np.frombuffer(small.data, dtype=np.uint8).copy()).to(dev.device)
    d_n = torch.tensor([small_r], dtype=torch.int64, device=dev.device)
    rc, (fields, res, sel) = held.call(patterns, rows=big_r, d_n_rows=d_n, bytes_len=small.bytes_len)
    rc2, want_res, want_sel, want_small = tmm.run_twin(tw, small, specs, capacity=big_r, rows=big_r, n_rows=small_r)
    assert rc == 0 and rc2 == 0 and want_res.code == 0 and 0 < want_res.n_matched and res == bytes(want_res) and sel == bytes(want_sel)
    d_res, d_sel, d_rec = tmm.expected(small, specs, capacity=big_r, R=small_r)
    assert tmm.res_fields(want_res) == d_res and want_small[:, :small_r].tobytes() == d_rec[:, :small_r].tobytes()
    exp = want_rec.copy()
    exp[:, :small_r] = want_small[:, :small_r]
    got = np.frombuffer(fields, dtype=tmm.FIELD)
    want = np.frombuffer(tms.with_canary(exp, len(specs), big_r), dtype=tmm.FIELD)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (int(bad[0]), got[bad[0]], want[bad[0]], int(bad.size))
