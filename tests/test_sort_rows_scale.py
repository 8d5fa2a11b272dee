"""msj_sort_rows_device (csrc/sort_rows_kernel.hip) past its grids and over arrays that an earlier call filled.

tests/test_sort_rows.py stops where one trip of every loop is enough but for the scan's.  Here:

  test_rows_past_the_grids     a row count just past each launch's grid, so that every loop takes a second trip: the full sort,
                               the selection chosen on the device with a limit of 10 and of 4 097 (it ends early there) and
                               forced to the key's last digit, a row list; against the twin byte for byte and against a
                               reference that shares nothing with it
  test_after_a_larger_call     small calls on tensors and a workspace that a larger call filled: live-looking records behind
                               R, row numbers behind N, keys and permutations in the workspace; every byte outside [0, K) of
                               d_order stays what the larger call left
  test_reference_on_cpu        the first test's inputs, the twin against the reference, without a GPU

The independent reference (reference(), below) is numpy's stable argsort over the values as x87 extended doubles, whose 64-bit
significand holds every int64 and every binary64 exactly, so that the compare is the compare of the reals; a row without a
value is +infinity, descending negates.  Nothing of sort_rows_math.h or of the twin is used.

The kernel's constants (csrc/sort_rows_kernel.hip) are named below as the shapes use them, written by hand: a constant changed
in the kernel has to be changed here too.
"""
import functools
import types

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from tests import test_sort_rows as tsr
from tests import test_sort_rows_math as tsm
from tests.test_sort_rows import dev, stw  # noqa: F401  (the fixtures)

B, T, S = tsr.B, tsr.T, tsr.S
ROW_GRID = 4096 * B                  # kRowBlocks = 4096 workgroups of sr_keys, sl_hist, sl_count, sl_place, sr_finish, `v += gridDim.x`
TILE_GRID = 1024 * T                 # kTileBlocks = 1024 workgroups of sr_count / sr_scatter, a tile each per trip
SCAN_CHUNK = S * T                   # the rows whose tiles fill one chunk of sr_scan
N_ROWS = ROW_GRID + B + 37           # 4 098 blocks of rows, 1 025 tiles: second trips everywhere, the last block holds 37 rows
TAIL = 300                           # live records behind R
DESC, VALUES_ONLY = tsr.DESC, tsr.VALUES_ONLY
L, D = tsr.L, tsr.D
FILL32 = tsr.FILL32
EXTENDED = np.finfo(np.longdouble).nmant >= 63      # (x86: the 80-bit format)


# ---- the independent reference -------------------------------------------------------------------------------------------------

def reference(col, R, rows_in=None, N=None, flags=0, limit=0):
    """-> (the first K row numbers as uint32, n_values): numpy alone"""
    seq = np.arange(R, dtype=np.int64) if rows_in is None else np.asarray(rows_in[:N], dtype=np.int64)
    inside = seq < R
    rec = col[np.where(inside, seq, 0)]
    number = inside & (rec["code"] == 0) & ((rec["type"] == L) | (rec["type"] == D)) & ((rec["flags"] & 64) == 0)
    with np.errstate(invalid="ignore"):
        as_double = rec["bits"].view(np.float64)
        number &= (rec["type"] == L) | np.isfinite(as_double)
        value = np.where(rec["type"] == L, rec["bits"].view(np.int64).astype(np.longdouble), as_double.astype(np.longdouble))
    key = np.where(number, -value if flags & DESC else value, np.longdouble(np.inf))
    order = np.argsort(key, kind="stable")
    M = int(number.sum()) if flags & VALUES_ONLY else len(seq)
    K = M if limit == 0 else min(limit, M)
    return seq[order[:K]].astype(np.uint32), int(number.sum())


def check_against_reference(want, col, R, rows_in, N, flags, limit, where):
    rows, n_values = reference(col, R, rows_in, N, flags, limit)
    assert want.res.n_values == n_values and want.res.n_written == len(rows), where
    bad = np.nonzero(want.order[:len(rows)] != rows)[0]
    assert bad.size == 0, (where, int(bad[0]), int(want.order[bad[0]]), int(rows[bad[0]]), int(bad.size))


# ---- the input -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def scale_columns():
    """name -> a column of N_ROWS + TAIL records.  "spread": ints of every size and doubles of every exponent, a few of them
    equal, one row in sixteen without a value; "ties": a thousand distinct small values, as int and as double, so that every cut
    falls inside a run of equal keys that every block holds a part of.  Behind N_ROWS: values below every row's"""
    rng = np.random.default_rng(2024)
    n = N_ROWS + TAIL
    k = np.arange(n)
    wide = rng.integers(-2**63, 2**63 - 1, n, endpoint=True) >> rng.integers(0, 64, n)
    spread = tsr.pick(k % 2 == 0, tsr.ints(wide), tsr.column(rng.integers(0, 2**64 - 1, n, dtype=np.uint64, endpoint=True) & np.uint64(0xFFEFFFFFFFFFFFFF), D))
    spread[k % 5 == 0] = spread[(k[k % 5 == 0] * 7) % 1000]      # equal values, far apart
    spread = tsr.without_values(spread, 16, 3)
    small = rng.integers(-500, 500, n)
    ties = tsr.without_values(tsr.pick(k % 3 == 0, tsr.doubles(small.astype(np.float64)), tsr.ints(small)), 50, 7)
    for col in (spread, ties):
        col[N_ROWS:] = tsr.doubles(np.full(TAIL, -1.7e308))
    return {"spread": spread, "ties": ties}


@functools.lru_cache(maxsize=1)
def scale_rows_in():
    """A row list just past the grids too: any order, repeats, entries at and past R"""
    rng = np.random.default_rng(7)
    rows = rng.integers(0, N_ROWS + 50, N_ROWS + 9).astype(np.uint32)
    rows[::1001] = 0xFFFFFFFF
    return rows


# what runs: (column, with the row list, flags, limit, modes)
CASES = [("spread", False, 0, 0, (0,)), ("spread", False, DESC, 10, (0, 2)), ("spread", False, 0, 4097, (0, 2)),
         ("ties", False, DESC, 0, (1,)), ("ties", False, 0, 10, (0, 2)), ("ties", False, DESC | VALUES_ONLY, 4097, (0, 2)),
         ("ties", True, 0, 4097, (0, 1, 2)), ("spread", True, VALUES_ONLY, 0, (0,))]


def case_input(case):
    name, listed, flags, limit, modes = case
    col = scale_columns()[name]
    rows_in = scale_rows_in() if listed else None
    return col, rows_in, (len(rows_in) - 9 if listed else None), flags, limit, modes


def test_constants():
    assert N_ROWS == 1_048_869 and (N_ROWS + B - 1) // B == 4096 + 2 and N_ROWS % B == 37 and (N_ROWS + T - 1) // T == 1024 + 1
    assert N_ROWS > ROW_GRID and N_ROWS > TILE_GRID and N_ROWS > SCAN_CHUNK
    sel = tsm.load_twin().srm_takes_selection
    assert sel(0, 10, N_ROWS) and sel(0, 4097, N_ROWS) and not sel(0, 0, N_ROWS)      # the path the device chooses for the limits below


@pytest.mark.skipif(not EXTENDED, reason="the reference needs a 64-bit significand")
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{'list-' if c[1] else ''}{c[2]}-{c[3]}")
def test_reference_on_cpu(case):
    """The scale input without a GPU: the twin against the reference"""
    col, rows_in, N, flags, limit, _ = case_input(case)
    want = tsm.twin_sort(tsm.load_twin(), col, N_ROWS, rows_in, N, flags, limit)
    assert want.rc == 0 and want.res.code == 0 and want.untouched()
    check_against_reference(want, col, N_ROWS, rows_in, N, flags, limit, case)
    if rows_in is None and limit:      # the cut falls among equal keys: the row behind it has the last row's value
        rows, _ = reference(col, N_ROWS, None, None, flags, limit + 1)
        assert case[0] != "ties" or col["bits"][rows[-1]].view(np.int64) == col["bits"][rows[-2]].view(np.int64) or col["type"][rows[-1]] != col["type"][rows[-2]]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{'list-' if c[1] else ''}{c[2]}-{c[3]}")
def test_rows_past_the_grids(dev, stw, case):
    """Second trips of every loop: the whole of d_order, the result and d_order_select are the twin's, and with them the
    reference's"""
    col, rows_in, N, flags, limit, modes = case_input(case)
    want = tsr.run_sort(dev, stw, col, N_ROWS, rows_in, N, flags, limit, where=case, modes=modes)
    assert want.res.code == 0 and want.res.n_rows == (N or N_ROWS) > ROW_GRID
    if EXTENDED:
        check_against_reference(want, col, N_ROWS, rows_in, N, flags, limit, case)


# ---- live-looking leftovers -------------------------------------------------------------------------------------------------

R1 = 5 * T + 300
STRIDE1, N1, CAP1 = R1 + 20, 4 * T + 11, 4 * T + 30
SMALL_N = [1, 63, 64, 65, 255, 256, 257, T + 1]


@functools.lru_cache(maxsize=1)
def larger_call():
    """(STRIDE1 records, CAP1 row numbers): values below anything a small call sorts in every record -- one read as a row
    would come first --, and valid row numbers in every entry of the list"""
    rng = np.random.default_rng(41)
    col = tsr.pick(np.arange(STRIDE1) % 2 == 0, tsr.doubles(-1e300 - rng.integers(0, 1000, STRIDE1) * 1e290), tsr.ints(tsm.INT64_MIN + rng.integers(0, 1000, STRIDE1)))
    return col, rng.integers(0, R1, CAP1).astype(np.uint32)


def smaller_call(n):
    """The larger call's arrays with n new records and n + 3 new list entries at the front"""
    col, rows = (x.copy() for x in larger_call())
    rng = np.random.default_rng(n)
    k = np.arange(n)
    col[:n] = tsr.without_values(tsr.pick(k % 2 == 0, tsr.ints(rng.integers(-40, 40, n)), tsr.doubles(rng.integers(-80, 80, n) * 0.5)), 6, 2)
    rows[:n + 3] = rng.integers(0, n + 2, n + 3)
    return col, rows


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL_N)
def test_after_a_larger_call(dev, stw, n):
    """One set of tensors, a call over R1 records and N1 listed rows, and then, with only the new rows written, calls over n
    rows: K entries of d_order are the twin's, and every other byte is what the larger call left"""
    import torch

    big_col, big_rows = larger_call()
    big = tsm.twin_sort(stw, big_col, R1, big_rows, N1, 0, 0, CAP1)
    assert big.rc == 0 and big.res.code == 0 and big.res.n_written == N1
    held = tsr.Held(dev, big_col, big_rows, CAP1)
    unlisted = types.SimpleNamespace(d_fields=held.d_fields, d_rows_in=None, t_order=held.t_order, t_res=held.t_res, t_sel=held.t_sel)
    col, rows = smaller_call(n)
    assert tsm.py_value(col[n])[0] is not None and rows[n + 3] < R1      # live behind R and behind N
    new_rows = lambda c, r: (held.d_fields[:n].copy_(torch.from_numpy(c[:n].view(np.int64).reshape(n, 2).copy())),
                             held.d_rows_in[:n + 3].copy_(torch.from_numpy(r[:n + 3].view(np.int32).copy())))
    for mode in tsr.MODES:
        for listed, flags, limit in ((False, 0, 0), (True, DESC, max(1, n // 2)), (True, VALUES_ONLY, n + 5), (False, DESC | VALUES_ONLY, 3)):
            new_rows(big_col, big_rows)
            before, res, _ = tsr.device_sort(dev, held, STRIDE1, R1, N1, 0, 0, CAP1, 0, 0, 1 if mode == 0 else mode)
            assert np.array_equal(before[:CAP1], big.order) and res.tobytes() == bytes(big.res), (n, mode, "the larger call")
            new_rows(col, rows)
            want = tsm.twin_sort(stw, col, n, rows if listed else None, n + 3 if listed else None, flags, limit, CAP1)
            assert want.rc == 0 and want.res.code == 0 and 0 < want.res.n_written <= n + 3
            after, res, sel = tsr.device_sort(dev, held if listed else unlisted, STRIDE1, n, n + 3, flags, limit, CAP1, 0, 0, mode)
            K = int(want.res.n_written)
            expected = before.copy()
            expected[:K] = want.order[:K]
            got = _lib.MsjSortRowsResult.from_buffer_copy(res.tobytes())
            assert res.tobytes() == bytes(want.res), (n, mode, listed, [(f, getattr(got, f), getattr(want.res, f)) for f, _ in got._fields_])
            assert sel.tobytes() == bytes(want.order_sel)
            bad = np.nonzero(after != expected)[0]
            assert bad.size == 0, (n, mode, listed, flags, limit, "entry", int(bad[0]), int(after[bad[0]]), int(expected[bad[0]]), int(bad.size), K)
