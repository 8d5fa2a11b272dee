"""msj_aggregate_device (csrc/aggregate_kernel.hip) past its grids and over arrays that an earlier call filled.

tests/test_aggregate.py stops at 17 blocks of rows and 4 097 groups: no workgroup of ag_pass1 / ag_pass2 makes a second trip
of its loop there, ag_init and ag_finish neither, the shipped switch between the LDS path and the global path never decides,
and behind the counts lies the fill, which is no number and no group.  Here:

  test_rows_past_the_row_grid        two trips and a third of 293 rows, at 1 .. 300 groups on both sides of the shipped switch,
                                     against the twin byte for byte and against a reference that shares nothing with it
  test_groups_past_the_group_grids   a million groups and a few hundred more, the accumulators dirty from another call
  test_after_a_larger_call           small calls on tensors that hold a larger call's records, codes and outputs
  test_reference_on_cpu              the first test's inputs, the twin against the reference, without a GPU

The independent reference (reference(), below) is numpy's grouping, ``math.fsum`` for a group's doubles, Python's ``int`` for
its int64s and numpy's minimum and maximum.  It equals the definition only where the definition cuts nothing: with E the
largest exponent of a group, a value's bits below 2^(E - 95) are dropped before the sum.  A double of exponent e has no bit
below 2^(e - 52), so a group whose exponents span at most 43 loses nothing, and its sum is the exact sum rounded once -- what
fsum returns.  The inputs keep every group's exponents within 40 of one another; reference() checks the span of every group
it is given and counts the groups it had to leave out, and the tests assert that this count is 0.

The kernel's constants (csrc/aggregate_kernel.hip) are named below as the shapes use them, written by hand: a constant changed
in the kernel has to be changed here too.  Device calls, the comparison over the whole record tensor and the fixtures are
tests/test_aggregate.py's, the twin is tests/test_aggregate_math.py's.

Tried once by hand on a copy of the kernel, on an MI355X (the tests that failed):
  the LDS zeroing of pass1 inside its trip loop     test_rows_past_the_row_grid with 1, 37, 255 and 256 groups and without codes
                                                    (257 and 300 groups never take the LDS path, and pass)
  ag_init's loop a single trip                      test_groups_past_the_group_grids (the result's flags: sums on top of sums)
  ag_finish's loop a single trip                    test_groups_past_the_group_grids (record 1 048 576 keeps the fill)
  `k <= h.R` for `k < h.R` in pass1                 every case of the three GPU tests
"""
import functools
import math
import random

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from mojo_simdjson_amd.document_stream import FIELD_DTYPE
from tests import test_aggregate as tag
from tests import test_aggregate_math as tam
from tests.test_aggregate import atw, dev  # noqa: F401  (the fixtures)

B = tag.B                            # kRows: rows per workgroup, one per lane
ROW_GRID = 2048 * B                  # kRowBlocks = 2048 workgroups of ag_pass1 / ag_pass2, `v += gridDim.x`
ACC_WORDS = 6                        # sizeof(Acc) / 16: the 16-byte words ag_init writes per group
INIT_GRID = 4096 * 256               # kGroupBlocks = 4096 workgroups of kThreads lanes: ag_init's words per trip
FINISH_GRID = 4096 * 256             # ... and ag_finish's groups per trip
SHIPPED = _lib.AGG_MAX_LDS_GROUPS    # kAggregateMaxLdsGroups, the switch as shipped
LIMITS = (SHIPPED, tag.LIMIT, 0)
INT32_MIN = -(2**31)
L, D = tam.L, tam.D
MASK = tam.MASK
SPAN = 43                            # the exponents of a group the definition sums without a cut: 95 - 52

R_ROWS = 2 * ROW_GRID + B + 37       # 4 098 blocks: workgroups 0 and 1 make three trips, the last block holds 37 rows
TAIL = 300                           # live records and codes behind R
ROW_CASES = [1, 37, 255, 256, 257, 300, None]     # G; None: one group and d_codes == NULL


def fields(bits, types, flags=0, code=0):
    """msj_field records from arrays of bits (uint64) and types"""
    out = np.zeros(len(bits), dtype=FIELD_DTYPE)
    out["bits"], out["type"], out["flags"], out["code"] = bits, types, flags, code
    return out


def double_patterns(rng, exponents):
    """Normal doubles of the given unbiased exponents (-1022 .. 1023), random significands and signs, as uint64 patterns"""
    n = len(exponents)
    biased = (np.asarray(exponents, dtype=np.int64) + 1023).astype(np.uint64)
    assert biased.min() >= 1 and biased.max() <= 2046
    return rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63) | biased << np.uint64(52) | rng.integers(0, 1 << 52, n, dtype=np.uint64)


def no_values(rng, recs, share, keep=None):
    """A share of the records made into what is no value: another type, a number without bits, an infinity, a NaN"""
    n = len(recs)
    pick = rng.random(n) < share
    if keep is not None:
        pick &= ~keep
    how = rng.integers(0, 4, n)
    recs["type"][pick & (how == 0)] = ord('"')
    recs["flags"][pick & (how == 1)] = tam.NO_BITS
    for j, pattern in ((2, 0x7FF0000000000000), (3, 0xFFF8000000000001)):
        m = pick & (how == j)
        recs["type"][m], recs["bits"][m] = D, pattern
    return recs


EXTREMES = np.array([(tam.double_bits(1e308), D), (tam.double_bits(-1e308), D), (tam.INT64_MIN & MASK, L), (tam.INT64_MAX, L)],
                    dtype=[("bits", "<u8"), ("type", "u1")])


def extreme_records(rng, n):
    """Values that no sum takes in unseen: +-1e308, INT64_MIN, INT64_MAX"""
    e = EXTREMES[rng.integers(0, len(EXTREMES), n)]
    return fields(e["bits"], e["type"])


# ---- the rows' input -----------------------------------------------------------------------------------------------------------

class Rows:
    """Two columns of R_ROWS records with a stride of R_ROWS + TAIL and a code per row.  roles: the groups with a part of
    their own (G >= 37), by name"""

    def __init__(self, G):
        rng = np.random.default_rng(9000 + G)
        R, n = R_ROWS, R_ROWS + TAIL
        self.G, self.R, self.stride = G, R, n
        roles = self.roles = dict(third_trip=G - 1, late_double=G - 2, int_overflow=G - 3, int_small=G - 4, run_a=0, run_b=1) if G >= 37 else {}
        spread = G - 2 if roles else G          # the random codes leave out the two groups whose rows have their places
        codes = rng.integers(0, spread, n).astype(np.int32)
        off = rng.random(n) < 0.05
        codes[off] = rng.choice(np.array([-1, G, INT32_MIN], dtype=np.int32), int(off.sum()))
        # whole waves of one group on both sides of a trip's border
        codes[ROW_GRID - 150:ROW_GRID + 150] = roles.get("run_a", 0)
        codes[2 * ROW_GRID - 150:2 * ROW_GRID + 150] = roles.get("run_b", 0)
        self.late_rows, self.n_third = None, 0
        if roles:
            # ints in the first trip, and a row each in the second and the third: column 0 has its double in the second and an
            # int in the third, column 1 the other way round
            ints = rng.choice(ROW_GRID - 200, 60, replace=False)
            self.late_rows = (ROW_GRID + 5000, 2 * ROW_GRID + 160)
            codes[ints] = codes[list(self.late_rows)] = roles["late_double"]
            behind_run = np.setdiff1d(np.arange(2 * ROW_GRID + 150, R), self.late_rows)
            third = np.union1d(rng.choice(behind_run, 40, replace=False), [2 * ROW_GRID + B, R - 37, R - 1])    # (the last block's rows among them)
            codes[third], self.n_third = roles["third_trip"], len(third)
        codes[R:] = rng.integers(0, G, TAIL)    # behind R: valid codes
        self.codes = codes
        self.columns = np.stack([self.column(rng, c) for c in range(2)])

    def column(self, rng, c):
        G, R, n, roles, codes = self.G, self.R, self.stride, self.roles, self.codes
        g = np.where((codes >= 0) & (codes < G), codes, 0)     # a row in no group has group 0's kind of value
        centres = rng.integers(-900, 901, G)
        bits = double_patterns(rng, centres[g] + rng.integers(-20, 21, n))
        types = np.full(n, D, dtype=np.uint8)
        if roles:
            big = rng.integers(0, 2**62, n, endpoint=True) * np.where(rng.random(n) < 0.75, 1, -1)
            for name, values in (("int_overflow", big), ("int_small", rng.integers(-10**6, 10**6 + 1, n)), ("late_double", rng.integers(-2**20, 2**20 + 1, n))):
                m = g == roles[name]
                bits[m], types[m] = values[m].astype(np.int64).view(np.uint64), L
            k = self.late_rows[c]      # exponent 30 and a last place of 2^-22: no integer, and beyond every int of the group on its side of zero
            bits[k], types[k] = double_patterns(rng, [30])[0] | np.uint64(1), D
        recs = no_values(rng, fields(bits, types), 0.03, keep=(g == roles["late_double"]) if roles else None)
        recs[R:] = extreme_records(rng, TAIL)
        return recs


@functools.lru_cache(maxsize=1)
def rows_case(G):
    """(Rows, d_codes or None, the reference) of a case of ROW_CASES"""
    rows = Rows(1 if G is None else G)
    codes = None if G is None else rows.codes
    return rows, codes, reference(rows.columns, rows.R, codes, rows.G)


# ---- the independent reference -------------------------------------------------------------------------------------------------

def exponent_span(doubles):
    """The largest less the smallest binary exponent of the non-zero finite doubles (0 for none)"""
    x = doubles[doubles != 0]
    if x.size == 0:
        return 0
    e = np.frexp(x)[1]
    return int(e.max() - e.min())


def reference(columns, R, codes, G):
    """-> (AGG_DTYPE records of shape (n_columns, G), the result's (flags, n_rows, n_groups, n_ungrouped, n_values, n_skipped),
    the non-empty groups left out because fsum is not the definition there).  Nothing of aggregate_math.h or of
    tests/test_aggregate_math.py's yardstick is used: numpy groups the rows, math.fsum adds doubles, int adds int64s"""
    group = np.zeros(R, dtype=np.int64) if codes is None else codes[:R].astype(np.int64)
    valid = (group >= 0) & (group < G)
    order = np.argsort(np.where(valid, group, G), kind="stable")
    counts = np.bincount(group[valid], minlength=G)
    starts = np.concatenate([[0], np.cumsum(counts)])
    n_valid = int(counts.sum())
    out = np.zeros((len(columns), G), dtype=tam.AGG_DTYPE)
    flags = n_values = n_skipped = left_out = 0
    for c, col in enumerate(columns):
        col = col[:R][order][:n_valid]
        number = (col["code"] == 0) & ((col["type"] == L) | (col["type"] == D))
        with np.errstate(invalid="ignore"):
            usable = number & ((col["flags"] & tam.NO_BITS) == 0) & ((col["type"] == L) | np.isfinite(col["bits"].view(np.float64)))
        n_skipped += int((number & ~usable).sum())
        for g in np.nonzero(counts)[0]:
            s = slice(starts[g], starts[g + 1])
            u = usable[s]
            types, bits = col["type"][s][u], col["bits"][s][u]
            rec = out[c, g]
            rec["n_rows"], rec["n_values"] = counts[g], len(bits)
            if len(bits) == 0:
                continue
            ints, doubles = bits[types == L].view(np.int64), bits[types == D].view(np.float64)
            if len(doubles) == 0:
                total = sum(ints.tolist())
                if tam.INT64_MIN <= total <= tam.INT64_MAX:
                    rec["sum_type"], rec["sum_bits"] = L, total & MASK
                else:
                    rec["sum_type"], rec["sum_bits"], rec["flags"] = D, tam.double_bits(float(total)), tam.INT_OVERFLOW
                rec["min_type"], rec["min_bits"], rec["max_type"], rec["max_bits"] = L, int(ints.min()) & MASK, L, int(ints.max()) & MASK
            else:
                every = np.concatenate([ints.astype(np.float64), doubles])
                if (len(ints) and int(np.abs(ints).max()) >= 2**53) or exponent_span(every) > SPAN:
                    left_out += 1
                    continue
                total = math.fsum(every.tolist())
                assert math.isfinite(total)
                rec["sum_type"], rec["sum_bits"] = D, tam.double_bits(total)
                lo, hi = min(ints.tolist() + doubles.tolist()), max(ints.tolist() + doubles.tolist())     # (int against float: exact in Python)
                assert len(ints) == 0 or not np.isin(doubles, every[:len(ints)]).any()      # no int equals a double: no tie to rule on
                rec["min_type"], rec["min_bits"] = (L, lo & MASK) if isinstance(lo, int) else (D, tam.double_bits(lo))
                rec["max_type"], rec["max_bits"] = (L, hi & MASK) if isinstance(hi, int) else (D, tam.double_bits(hi))
            flags |= int(rec["flags"])
        n_values += int(out[c]["n_values"].sum())
    return out, (flags, R, G, R - n_valid, n_values, n_skipped), left_out


def check_against_reference(got, rows, ref, where):
    """got: a tam.Agg of the case -- every group's record and the result are the reference's, and no group was left out"""
    want, result, left_out = ref
    G = rows.G
    assert left_out == 0, (where, left_out)
    records = got.records(G)
    bad = np.nonzero(records != want)
    assert bad[0].size == 0, (where, int(bad[0][0]), int(bad[1][0]), records[bad][0], want[bad][0], int(bad[0].size))
    assert got.result() == result, (where, got.result(), result)
    # the input is what the test is named for
    assert (want["n_values"] > 0).all() and (want["sum_type"][:, 0] == D).all() and result[5] > 1000
    if rows.roles:
        r = rows.roles
        assert result[0] == tam.INT_OVERFLOW and result[3] > R_ROWS // 40
        assert (want["flags"][:, r["int_overflow"]] == tam.INT_OVERFLOW).all() and (want["sum_type"][:, r["int_overflow"]] == D).all()
        assert (want["sum_type"][:, r["int_small"]] == L).all() and (want["flags"][:, r["int_small"]] == 0).all()
        assert rows.n_third >= 40 and (want["n_rows"][:, r["third_trip"]] == rows.n_third).all() and (want["n_rows"][:, r["late_double"]] == 62).all()
        late = want[:, r["late_double"]]      # (its one double is the minimum or the maximum, by its sign)
        assert (late["sum_type"] == D).all() and (late["n_values"] == 62).all() and ((late["min_type"] == D) ^ (late["max_type"] == D)).all()
        assert (want["n_rows"][:, r["run_a"]] >= 300).all() and (want["n_rows"][:, r["run_b"]] >= 300).all()


@pytest.mark.parametrize("G", ROW_CASES)
def test_reference_on_cpu(atw, G):
    """The rows' input without a GPU: the twin, with the minimum and the maximum found either way, against the reference in
    every group"""
    assert R_ROWS == 1_048_869 and (R_ROWS + B - 1) // B == 2 * 2048 + 2 and R_ROWS % B == 37 and R_ROWS % tag.WAVE != 0
    rows, codes, ref = rows_case(G)
    for split in (0, 1):
        got = tam.twin_aggregate(atw, rows.columns, rows.R, codes, rows.G, capacity=rows.G + 2, split=split)
        assert got.rc == 0 and got.res.code == 0
        check_against_reference(got, rows, ref, ("twin", G, split))


# ---- 1 and 2: rows past the row grid ------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("G", ROW_CASES)
def test_rows_past_the_row_grid(dev, atw, G):
    """Three trips of ag_pass1 / ag_pass2 at the shipped limit, at 8 and with the LDS path off: the whole record tensor and
    the result are the twin's, and with them the reference's"""
    rows, codes, ref = rows_case(G)
    held = tag.Held(dev, rows.columns, codes, rows.G + 2)
    want = tag.run_aggregate(dev, atw, rows.columns, rows.R, codes, rows.G, where=("rows", G), limits=LIMITS, held=held)
    assert want.res.code == 0 and want.res.n_rows == R_ROWS > 2 * ROW_GRID + B
    check_against_reference(want, rows, ref, ("device", G))


# ---- 3: groups past the group grids -------------------------------------------------------------------------------------------

G_GROUPS = 4096 * 256 + 300
R_GROUPS = 200_003
FIRST_INIT = INIT_GRID // ACC_WORDS      # 174 762: the group whose words ag_init's first trip ends in
BORDERS = [FIRST_INIT - 1, FIRST_INIT, FIRST_INIT + 1, FIRST_INIT + 2, FINISH_GRID - 1, FINISH_GRID, FINISH_GRID + 1, FINISH_GRID + 2, G_GROUPS - 1]


def wild_records(rng, n):
    """Records of every kind: int64s of every length, doubles of every exponent (a few of them not finite), and no values"""
    ints = rng.integers(-2**63, 2**63 - 1, n, endpoint=True) >> rng.integers(0, 64, n)
    bits = np.where(rng.random(n) < 0.5, ints.view(np.uint64), rng.integers(0, 2**64 - 1, n, dtype=np.uint64, endpoint=True))
    types = np.where(bits == ints.view(np.uint64), L, D).astype(np.uint8)
    return no_values(rng, fields(bits, types), 0.05)


def group_rows(seed):
    """One column of R_GROUPS records, and codes that are spread over all G_GROUPS groups with three rows in each of BORDERS"""
    rng = np.random.default_rng(seed)
    n = R_GROUPS + 8
    codes = rng.integers(0, G_GROUPS, n).astype(np.int32)
    off = rng.random(n) < 0.03
    codes[off] = rng.choice(np.array([-1, G_GROUPS, INT32_MIN], dtype=np.int32), int(off.sum()))
    places = rng.choice(R_GROUPS, 3 * len(BORDERS), replace=False)
    codes[places] = np.repeat(BORDERS, 3)
    recs = wild_records(rng, n)
    recs["type"][places[::3]], recs["flags"][places[::3]] = L, 0      # (at least a value in each)
    return recs, codes


def groups_hit(codes):
    valid = (codes[:R_GROUPS] >= 0) & (codes[:R_GROUPS] < G_GROUPS)
    return np.bincount(codes[:R_GROUPS][valid], minlength=G_GROUPS) > 0


@pytest.mark.gpu
def test_groups_past_the_group_grids(dev, atw):
    """ag_init's and ag_finish's second trips.  Before each compared call another call with other records and other codes has
    left its sums in the context's accumulators: the groups that only that call gave rows come out all zero"""
    assert FIRST_INIT == 174_762 and FINISH_GRID == 1_048_576 and G_GROUPS == 1_048_876 and BORDERS[-1] > FINISH_GRID + 2
    first, first_codes = group_rows(31)
    second, second_codes = group_rows(32)
    only_first = groups_hit(first_codes) & ~groups_hit(second_codes)
    assert int(only_first[FIRST_INIT + 1:].sum()) >= 1000 and int(only_first[FINISH_GRID:].sum()) >= 10
    assert groups_hit(second_codes)[BORDERS].all() and groups_hit(first_codes)[BORDERS].all()
    capacity = G_GROUPS + 2
    dirt = tag.Held(dev, first, first_codes, capacity)
    held = tag.Held(dev, second, second_codes, capacity)
    for limit in (SHIPPED, 0):      # (the global path both times: G is far above any limit)
        groups, res = tag.device_aggregate(dev, first, R_GROUPS, first_codes, G_GROUPS, capacity, limit=limit, held=dirt)
        got = groups[:48 * G_GROUPS].view(tam.AGG_DTYPE)
        assert _lib.MsjAggregateResult.from_buffer_copy(res.tobytes()).code == 0 and (got["n_rows"][only_first] > 0).all()
        want = tag.run_aggregate(dev, atw, second, R_GROUPS, second_codes, G_GROUPS, capacity=capacity, where=("groups", limit), limits=(limit,), held=held)
        records = want.records(G_GROUPS)[0]
        assert want.res.code == 0 and want.res.n_groups == G_GROUPS and want.res.n_values > R_GROUPS // 2
        assert not records[only_first].view(np.uint8).any()      # (the twin's, and byte for byte the device's)
        assert (records["n_rows"][BORDERS] >= 3).all() and (records["n_values"][BORDERS] >= 1).all()


# ---- 4: live-looking leftovers -------------------------------------------------------------------------------------------------

R1, G1 = 3 * B + 300, 64
STRIDE1, CAPACITY1 = R1 + 20, G1 + 2
SMALL_R = [1, 63, 64, 65, 255, 256, 257]
SMALL_G = [1, 7, 9, 40]


@functools.lru_cache(maxsize=1)
def larger_call():
    """(two columns of STRIDE1 records, codes): extreme values in every row, valid codes of G1 groups, half of them 0 --
    and 0 in each row that is the first behind a small call's rows, a valid code for every G"""
    rng = np.random.default_rng(41)
    columns = np.stack([extreme_records(rng, STRIDE1) for _ in range(2)])
    codes = np.where(rng.random(STRIDE1) < 0.5, 0, rng.integers(0, G1, STRIDE1)).astype(np.int32)
    codes[SMALL_R] = 0
    return columns, codes


def smaller_call(R, G):
    """The larger call's arrays with R new rows at the front: mixed records, codes in [0, G) and, in some rows, codes of the
    larger dictionary, G .. G1 - 1, and -1"""
    columns, codes = (x.copy() for x in larger_call())
    rng = random.Random(100 * R + G)
    centres = [rng.randrange(0, 2047) for _ in range(G)]
    for k in range(R):
        g = rng.randrange(G)
        codes[k] = g if rng.random() < 0.8 else rng.choice([-1, G, G1 - 1, rng.randrange(G, G1)])
        for c in range(2):
            columns[c, k] = tam.record(tam.random_value(rng, centres[g]))
    return columns, codes


@pytest.mark.gpu
@pytest.mark.parametrize("R", SMALL_R)
def test_after_a_larger_call(dev, atw, R):
    """One set of tensors, a call of R1 rows and G1 groups, and then, with only the new rows written, a call of R rows and G
    groups read through d_n_groups: G records per column are the twin's, and every other byte is what the larger call left"""
    big_columns, big_codes = larger_call()
    big = tam.twin_aggregate(atw, big_columns, R1, big_codes, G1, capacity=CAPACITY1)
    big_res = np.frombuffer(bytes(big.res), dtype=np.uint8)
    assert big.rc == 0 and big.res.code == 0 and big.res.n_values == 2 * R1
    held = tag.Held(dev, big_columns, big_codes, CAPACITY1)
    for G in SMALL_G:
        columns, codes = smaller_call(R, G)
        want = tam.twin_aggregate(atw, columns, R, codes, G, capacity=CAPACITY1)
        assert want.rc == 0 and want.res.code == 0
        py_records, py_result = tam.py_aggregate(columns, R, codes, G)
        assert np.array_equal(want.records(G), py_records) and want.result() == py_result, (R, G)
        assert R < 63 or (py_result[3] > 0 and ((codes[:R] >= G) & (codes[:R] < G1)).any())
        assert 0 <= codes[R] < G and tam.py_value(tuple(int(x) for x in columns[0, R])) is not None     # live behind R
        want_res = np.frombuffer(bytes(want.res), dtype=np.uint8)
        mine = np.zeros(len(big.groups), dtype=bool)      # the bytes the small call owns
        for c in range(2):
            mine[48 * c * CAPACITY1:48 * (c * CAPACITY1 + G)] = True
        assert (want.groups[~mine] == tam.FILL).all()
        for limit in LIMITS:
            held.write_rows(big_columns, big_codes)
            groups, res = tag.device_aggregate(dev, None, R1, None, G1, CAPACITY1, by_pointer=True, limit=limit, held=held)
            assert np.array_equal(groups[:len(big.groups)], big.groups) and (groups[len(big.groups):] == tam.FILL).all(), (R, G, limit, "the larger call")
            assert np.array_equal(res, big_res)
            held.write_rows(columns[:, :R], codes[:R])
            after, res = tag.device_aggregate(dev, None, R, None, G, CAPACITY1, by_pointer=True, limit=limit, held=held)
            expected = groups.copy()
            expected[:len(big.groups)][mine] = want.groups[mine]
            got = _lib.MsjAggregateResult.from_buffer_copy(res.tobytes())
            assert np.array_equal(res, want_res), (R, G, limit, [(n, getattr(got, n), getattr(want.res, n)) for n, _ in got._fields_])
            bad = np.nonzero(after != expected)[0]
            assert bad.size == 0, (R, G, limit, "record", int(bad[0]) // 48, after[48 * (int(bad[0]) // 48):][:48].view(tam.AGG_DTYPE),
                                   expected[48 * (int(bad[0]) // 48):][:48].view(tam.AGG_DTYPE), int(bad.size))
