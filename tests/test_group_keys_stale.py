"""msj_bucket_rows_device and msj_group_keys_device on arrays that hold a larger call's leftovers (the manner of
tests/test_stale_tails.py): a call over 600 rows runs first, in one context; then, in the SAME tensors and the same context --
its workspace holds the larger call's counters -- a call over 257 rows whose first 257 records and codes are new and whose
arrays go on behind R with the larger call's live-looking records and codes.  Expected: the smaller call's outputs from the
host twin up to R (R + 1 offsets, R * W key bytes), the LARGER call's bytes untouched behind them, and results that count
the smaller call alone."""
import random

import numpy as np
import pytest

from tests import test_group_keys as tgk
from tests import test_group_keys_math as tgm
from tests import test_tape_documents as ttd

pytestmark = pytest.mark.gpu

BIG, SMALL = 600, 257

dev = tgk.dev
gtw = tgk.gtw


def raw(x):
    return np.frombuffer(np.ascontiguousarray(x).tobytes(), dtype=np.uint8)


def test_keys_in_a_larger_calls_arrays(dev, gtw):
    import torch

    rng = random.Random(4)
    kinds = [tgm.NUMBER, tgm.CODE, tgm.NUMBER]
    flags = [0, tgm.NULL_IS_GROUP, 0]
    W = 27
    big = tgm.random_parts(rng, kinds, BIG, flags)
    fresh = tgm.random_parts(rng, kinds, SMALL, flags)
    small = [tgm.Part(np.concatenate([f.column, b.column[SMALL:]]), f.flags) for f, b in zip(fresh, big)]
    want_big = tgm.twin_keys(gtw, big, BIG)
    want_small = tgm.twin_keys(gtw, small, SMALL)
    assert want_big.res.code == want_small.res.code == 0 and want_big.res.n_keys != want_small.res.n_keys

    columns = [ttd.to_device(dev, p.column) for p in big]
    d_off, d_valid, d_bytes = tgk.filled(dev, 8 * (BIG + 1)), tgk.filled(dev, BIG), tgk.filled(dev, BIG * W)
    d_res = tgk.filled(dev, 48)

    def call(parts, R):
        for c, p in zip(columns, parts):
            c.copy_(ttd.to_device(dev, p.column))
        arr = tgm.part_array(parts, [c.data_ptr() for c in columns])
        d_sel = tgk.select_tensor(dev, R)
        assert dev.lib.msj_group_keys_device(dev.ctx, arr, len(parts), BIG, d_sel.data_ptr(), d_off.data_ptr(), d_valid.data_ptr(), d_bytes.data_ptr(),
                                             BIG, BIG * W, d_res.data_ptr(), dev._stream()) == 0
        torch.cuda.synchronize()

    call(big, BIG)
    tgk.same(d_bytes, tgk.with_canary(want_big.bytes, BIG * W), "the larger call's key bytes")
    call(small, SMALL)
    tgk.same(d_res, tgk.with_canary(raw(bytes(want_small.res)), 48), "the result")
    offsets = want_big.offsets.copy()
    offsets[:SMALL + 1] = want_small.offsets[:SMALL + 1]
    valid, data = want_big.valid.copy(), want_big.bytes.copy()
    valid[:SMALL], data[:SMALL * W] = want_small.valid[:SMALL], want_small.bytes[:SMALL * W]
    tgk.same(d_off, tgk.with_canary(offsets, 8 * (BIG + 1)), "the offsets")
    tgk.same(d_valid, tgk.with_canary(valid, BIG), "the valid bytes")
    tgk.same(d_bytes, tgk.with_canary(data, BIG * W), "the key bytes")


def test_bucket_in_a_larger_calls_arrays(dev, gtw):
    import torch

    big = tgk.bucket_rows_of(random.Random(5), BIG)
    small = np.concatenate([tgk.bucket_rows_of(random.Random(6), SMALL), big[SMALL:]])
    want_big = tgm.twin_bucket(gtw, big, BIG, 60000, 11)
    want_small = tgm.twin_bucket(gtw, small, SMALL, 60000, 11)
    assert want_big.res.n_bucketed != want_small.res.n_bucketed
    d_rows = ttd.to_device(dev, big)
    d_out, d_res, d_osel = tgk.filled(dev, 16 * BIG), tgk.filled(dev, 48), tgk.filled(dev, 48)

    def call(rows, R):
        d_rows.copy_(ttd.to_device(dev, rows))
        d_sel = tgk.select_tensor(dev, R)
        assert dev.lib.msj_bucket_rows_device(dev.ctx, d_rows.data_ptr(), d_sel.data_ptr(), 60000, 11, 0, d_out.data_ptr(), BIG, d_res.data_ptr(),
                                              d_osel.data_ptr(), dev._stream()) == 0
        torch.cuda.synchronize()

    call(big, BIG)
    tgk.same(d_out, tgk.with_canary(want_big.out, 16 * BIG), "the larger call's records")
    call(small, SMALL)
    out = want_big.out.copy()
    out[:SMALL] = want_small.out[:SMALL]
    tgk.same(d_out, tgk.with_canary(out, 16 * BIG), "the records")
    tgk.same(d_res, tgk.with_canary(raw(bytes(want_small.res)), 48), "the result")
    tgk.same(d_osel, tgk.with_canary(raw(bytes(want_small.out_sel)), 48), "the output's select result")
