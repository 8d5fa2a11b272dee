"""One dictionary across windows on the device (msj_dictionary_extend_device, csrc/dictionary_extend_kernel.hip).

Expected values come from the host twin of the same arithmetic (tests/dictionary_extend_math_host.cpp), which
tests/test_dictionary_extend_math.py holds against the definition written in Python.  The device runs against the twin over
the WHOLE of every array: both start from the same fill, with 64 bytes of canary behind each capacity and the prior part in
place, so a store into the prior part, past a capacity or one the twin does not make shows.  max_probe, which depends on
which item reached a slot first, is held against its bounds.  The end-to-end test runs the real chain through
DocumentStream with RunningDictionary.

The kernels' constants (csrc/dictionary_extend_kernel.hip, as built) are named below as the shapes use them.
"""
import json

import numpy as np
import pytest

from tests import test_dictionary as tdg
from tests import test_dictionary_extend_math as txm
from tests import test_dictionary_math as tdc
from tests import test_validate_documents as tvd
from tests.test_dictionary_extend_math import FROZEN, NO_ENTRY, Arrays, arrays_of, summary
from tests.test_dictionary_math import FILL, MSJ_CAPACITY, WEAK, column_of

pytestmark = pytest.mark.gpu

B = 256                  # kRows: ITEMS (prior entries, then rows) per workgroup of the kernels over the items
ROW_GRID = 4096 * B      # kGridBlocks = 4096 blocks of kRows items, `v += gridDim.x`
SCAN_CHUNK = 1024        # wave_ops.h, scan_in_place: blocks per chunk of the running sums
LONG_ITEM = 512          # kLongItem: an item of MORE bytes than this is hashed and compared by a wave, not by its lane
LONG_CAP = 1024          # kLongCap: entries of the list of long items; a long item past it is carried by its own wave
PIECE = 16384            # kPiece: bytes of aligned output a workgroup of dx_copy takes at a time
BAD_ARGUMENT = -1


@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    d = Stage1Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def xtwin():
    return txm.load_twin()


def device_extend(dev, a, arrays, P, flags=0, n_rows=None, p_word=None, shift=0, d_codes=None, d_result=None, sync=True):
    """msj_dictionary_extend_device over an uploaded column and a copy of the Arrays (None: layout-only), uploaded with their
    fill and canaries; n_rows / p_word: the counts as words on the device; shift: d_dict_bytes starts that many bytes off a
    16-byte boundary -> (result, codes with canary, the Arrays as the device left them)"""
    import torch

    up = lambda x: torch.from_numpy(x).to(dev.device)
    t_codes = up(txm.filled_codes(a.rows)) if d_codes is None else d_codes
    t_off = t_first = t_all = t_bytes = None
    if arrays is not None:
        t_off, t_first = up(arrays.offsets.view(np.int64)), up(arrays.first.view(np.int32))
        t_all = up(np.concatenate([np.full(shift, FILL, dtype=np.uint8), arrays.bytes]))
        t_bytes = t_all[shift:]
    word = lambda v: up(np.array([v], dtype=np.uint64).view(np.int64)) if v is not None else None
    res, *_ = dev.dictionary_extend(a.d_offsets, a.d_bytes, a.d_valid, t_off, t_first, t_bytes, n_prior=P, d_n_prior=word(p_word), rows=a.rows,
                                    d_n_rows=word(n_rows), bytes_len=a.bytes_len, d_codes=t_codes,
                                    dict_capacity=arrays.dict_capacity if arrays else None,
                                    dict_bytes_capacity=arrays.dict_bytes_capacity if arrays else None, frozen=bool(flags & FROZEN),
                                    weak_hash=bool(flags & WEAK), d_result=d_result, sync=sync)
    if not sync:
        return res, t_codes, (t_off, t_first, t_all)
    left = None
    if arrays is not None:
        assert bool((t_all[:shift] == FILL).all())
        left = arrays.copy()
        left.offsets, left.first, left.bytes = t_off.cpu().numpy().view(np.uint64), t_first.cpu().numpy().view(np.uint32), t_bytes.cpu().numpy()
    return res, t_codes.cpu().numpy(), left


def same(got, want, slots, where=None):
    """(result, codes, Arrays) of the device and of the twin: every member but max_probe, every array whole"""
    (res, codes, left), (wres, wcodes, wleft) = got, want
    assert summary(res) == summary(wres), (where, summary(res), summary(wres))
    longest = int(res.max_probe)
    assert (longest == 0) == (wres.max_probe == 0) and longest <= slots, (where, longest, slots)
    pairs = [("codes", codes, wcodes)]
    if wleft is not None:
        pairs += [(name, getattr(left, name), getattr(wleft, name)) for name in ("offsets", "first", "bytes")]
    for name, x, y in pairs:
        bad = np.nonzero(x != y)[0]
        assert bad.size == 0, (where, name, int(bad[0]), x[bad[:4]].tolist(), y[bad[:4]].tolist(), bad.size)


def check(dev, xtwin, col, arrays, P, flags=(0,), shift=0, where=None, a=None, n_rows=None, p_word=None):
    """The device against the twin from the same Arrays -> the last (twin result, codes, Arrays as left)"""
    a = tdg.OnDevice(dev, col) if a is None else a
    for f in flags:
        wleft = arrays.copy() if arrays is not None else None
        wres, wcodes = txm.twin_extend(xtwin, col, wleft, 0 if p_word is not None else P, f, n_rows=n_rows, p_word=p_word)
        got = device_extend(dev, a, arrays, 0 if p_word is not None else P, f, n_rows=n_rows, p_word=p_word, shift=shift)
        R = col.rows if n_rows is None else n_rows
        same(got, (wres, wcodes, wleft), xtwin.dxm_extend_slots(P if p_word is None else p_word, R, f) if wres.max_probe else 0, (where, f))
    return wres, wcodes, wleft


def numbered_prior(n, width=7, spare=(0, 0)):
    """n distinct prior entries of `width` decimal digits (tests/test_dictionary.py's ``numbered``) -> Arrays"""
    col = tdg.numbered(n, width)
    return Arrays(col.offsets, col.data.tobytes(), n + spare[0], width * n + spare[1])


# ---- borders ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [0, 1, B - 1, B, B + 1])
def test_item_counts(dev, xtwin, P):
    """P and R in {0, 1, 255, 256, 257}: both kinds of item cross a block border.  Values repeat with a period that divides
    neither; null rows, and "" as a prior entry and as a new value; both hashes; unfrozen and frozen."""
    for R in (0, 1, B - 1, B, B + 1):
        prior = [b"" if c == 3 else b"value-%d" % c for c in range(P)]
        values = [None if k % 11 == 5 else b"" if k % 7 == 3 else b"value-%d" % (k * 5 % 37 * 9) for k in range(R)]
        arrays = arrays_of(prior, spare=(R + 1, 12 * R + 3))
        wres, _, _ = check(dev, xtwin, column_of(values), arrays, P, flags=(0, WEAK, FROZEN, FROZEN | WEAK), shift=(P + R) % 16, where=(P, R))
        assert wres.n_prior == P and wres.n_rows == R
    if P == 0:
        check(dev, xtwin, column_of(values), None, 0, flags=(0, WEAK), where="layout-only")


# ---- the two identities -----------------------------------------------------------------------------------------------------

def test_without_prior_it_is_the_dictionary_call(dev):
    """P = 0 against dev.dictionary on the same column: every array and every shared member, the extra members 0."""
    import torch

    values = txm.generated(21, 3 * B + 9)
    col = column_of(values)
    a = tdg.OnDevice(dev, col)
    res, d_codes, d_off, d_first, d_bytes = dev.dictionary(a.d_offsets, a.d_bytes, a.d_valid, rows=a.rows, bytes_len=a.bytes_len)
    n, total = int(res.n_distinct), int(res.dict_bytes)
    x_off, x_first, x_bytes = torch.zeros_like(d_off), torch.zeros_like(d_first), torch.zeros_like(d_bytes)
    xres, x_codes, *_ = dev.dictionary_extend(a.d_offsets, a.d_bytes, a.d_valid, x_off, x_first, x_bytes, rows=a.rows, bytes_len=a.bytes_len,
                                              dict_capacity=n, dict_bytes_capacity=total)
    assert summary(xres) == (res.code, res.flags, res.n_rows, res.n_values, n, total, 0, 0) and res.code == 0
    assert torch.equal(x_codes[:a.rows], d_codes[:a.rows]) and torch.equal(x_off[:n + 1], d_off[:n + 1])
    assert torch.equal(x_first[:n], d_first[:n]) and torch.equal(x_bytes[:total], d_bytes[:total])


def test_a_chain_on_the_device_is_the_whole_column(dev):
    """Four windows (300, 1, 0 and 513 rows) against one dev.dictionary over the concatenation: each call's P is the previous
    result's n_distinct ON THE DEVICE (d_n_prior), all enqueued with sync=False, nothing waited for until the end."""
    import torch

    sizes = (300, 1, 0, 513)
    values = txm.generated(22, sum(sizes), vocabulary=120)
    whole = tdg.OnDevice(dev, column_of(values))
    res, d_codes, d_off, d_first, d_bytes = dev.dictionary(whole.d_offsets, whole.d_bytes, whole.d_valid, rows=whole.rows, bytes_len=whole.bytes_len)
    n, total = int(res.n_distinct), int(res.dict_bytes)
    windows, at = [], 0
    for size in sizes:
        windows.append(tdg.OnDevice(dev, column_of(values[at:at + size])))
        at += size
    x_off = torch.full((n + 1,), 0x77, dtype=torch.int64, device=dev.device)
    x_first = torch.full((n,), 0x77, dtype=torch.int32, device=dev.device)
    x_bytes = torch.full((total,), 0x77, dtype=torch.uint8, device=dev.device)
    results = [torch.zeros(64, dtype=torch.uint8, device=dev.device) for _ in sizes]
    codes = [torch.full((max(size, 1),), 0x77, dtype=torch.int32, device=dev.device) for size in sizes]
    torch.cuda.synchronize()
    for j, w in enumerate(windows):
        d_n_prior = results[j - 1][24:32].view(torch.int64) if j else None
        dev.dictionary_extend(w.d_offsets, w.d_bytes, w.d_valid, x_off, x_first, x_bytes, d_n_prior=d_n_prior, rows=w.rows, bytes_len=w.bytes_len,
                              d_codes=codes[j], dict_capacity=n, dict_bytes_capacity=total, d_result=results[j], sync=False)
    torch.cuda.synchronize()
    from mojo_simdjson_amd import _lib

    got = [_lib.MsjDictionaryExtendResult.from_buffer_copy(r.cpu().numpy().tobytes()) for r in results]
    assert all(r.code == 0 for r in got) and [r.n_rows for r in got] == list(sizes) and got[-1].n_distinct == n and got[-1].dict_bytes == total
    assert [r.n_prior for r in got] == [0] + [r.n_distinct for r in got[:-1]]
    assert torch.equal(torch.cat([c[:size] for c, size in zip(codes, sizes)]), d_codes[:whole.rows])
    assert torch.equal(x_off, d_off[:n + 1]) and torch.equal(x_bytes, d_bytes[:total])
    row_base = torch.zeros(n, dtype=torch.int32, device=dev.device)
    at = 0
    for r, size in zip(got, sizes):
        row_base[r.n_prior:r.n_distinct] = at
        at += size
    assert torch.equal(x_first + row_base, d_first[:n])


# ---- the copy ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("residue", range(16))
def test_base_at_every_residue(dev, xtwin, residue):
    """base at every residue of 16, d_dict_bytes 0 .. 15 bytes off a 16-byte boundary for a few of them: the bytes below
    base are untouched (the whole array is the twin's), the bytes from base on are the new values'."""
    prior = [b"p" * (16 + residue), b"q"]   # base = 17 + residue
    values = [b"new-%d-" % k + bytes([97 + k % 26]) * (k % 40) for k in range(90)] + [b"q", None, b"p" * (16 + residue)]
    arrays = arrays_of(prior, spare=(95, 4000))
    col = column_of(values)
    a = tdg.OnDevice(dev, col)
    shifts = range(16) if residue in (0, 7, 15) else (0, (5 * residue) % 16)
    for shift in shifts:
        wres, _, left = check(dev, xtwin, col, arrays, 2, shift=shift, a=a, where=(residue, shift))
        assert wres.n_matched == 2 and int(arrays.offsets[2]) % 16 == (17 + residue) % 16
        assert left.bytes[:17 + residue].tobytes() == b"".join(prior)


# ---- long values ------------------------------------------------------------------------------------------------------------

def test_items_around_the_long_threshold(dev, xtwin):
    """Lengths 511 .. 514 as prior entry and as row: equal pairs, and pairs that differ in the last byte."""
    prior, values = [], []
    for n in (LONG_ITEM - 1, LONG_ITEM, LONG_ITEM + 1, LONG_ITEM + 2):
        base = bytes((3 * j + n) & 0xFF for j in range(n))
        prior += [base, b"p%d" % n]
        values += [base, b"short", base[:-1] + b"\xff", None, base, b"", base[:-1] + b"\xff"]
    arrays = arrays_of(prior, spare=(8, 4 * 520 + 8))
    wres, wcodes, _ = check(dev, xtwin, column_of(values), arrays, len(prior), flags=(0, WEAK, FROZEN), shift=3)
    assert wres.n_matched == 8 and wcodes[:7].tolist() == [0, NO_ENTRY, NO_ENTRY, -1, 0, NO_ENTRY, NO_ENTRY]


def test_one_mebibyte_prior_entry(dev, xtwin):
    """A 1 MiB prior entry met by an equal row and by one that differs in its last byte."""
    rng = np.random.default_rng(31)
    big = rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    other = big[:-1] + bytes([big[-1] ^ 1])
    arrays = arrays_of([b"x", big], spare=(2, (1 << 20) + 5))
    wres, wcodes, _ = check(dev, xtwin, column_of([other, big, b"x", other]), arrays, 2, flags=(0, FROZEN), shift=9)
    assert wcodes[:4].tolist() == [NO_ENTRY, 1, 0, NO_ENTRY]
    wres, wcodes, _ = check(dev, xtwin, column_of([other, big, b"x", other]), arrays, 2, shift=9)
    assert wcodes[:4].tolist() == [2, 1, 0, 2] and wres.dict_bytes == 2 * (1 << 20) + 1 > 100 * PIECE


@pytest.mark.parametrize("long_prior", [LONG_CAP + 40, 40])
def test_long_item_list_from_either_side(dev, xtwin, long_prior):
    """More long items than the list holds, split between prior entries and rows: with 1 064 long prior entries the list
    fills before the rows, with 40 the rows fill it and some find it full.  Every third long row repeats a prior entry."""
    long_rows = LONG_CAP + 80 - long_prior
    make = lambda j: b"%06d" % j + bytes([65 + j % 26]) * (LONG_ITEM - 5 + j % 9)
    prior = [x for c in range(long_prior) for x in (make(c), b"s%d" % c)]
    values = [x for k in range(long_rows) for x in (make(k % long_prior if k % 3 == 2 else 5000 + k), b"s%d" % (k % 50))]
    assert sum(len(v) > LONG_ITEM for v in prior + values) == LONG_CAP + 80
    arrays = arrays_of(prior, spare=(long_rows + 60, (LONG_ITEM + 12) * long_rows + 600))
    wres, _, _ = check(dev, xtwin, column_of(values), arrays, len(prior), flags=(0, FROZEN), where=long_prior)
    assert wres.n_matched >= long_rows // 3


# ---- contention -------------------------------------------------------------------------------------------------------------

def test_hot_column_is_reproducible(dev, xtwin):
    """70 000 rows over three values of which two are prior entries, run twice: bit-identical, and the twin's."""
    names = (b"active", b"suspended", b"closed")
    col = column_of([names[k % 3] for k in range(70000)])
    a = tdg.OnDevice(dev, col)
    arrays = arrays_of([b"closed", b"unused", b"active"], spare=(2, 20))
    wleft = arrays.copy()
    wres, wcodes = txm.twin_extend(xtwin, col, wleft, 3)
    runs = [device_extend(dev, a, arrays, 3, shift=1) for _ in range(2)]
    for got in runs:
        same(got, (wres, wcodes, wleft), xtwin.dxm_extend_slots(3, 70000, 0))
    assert runs[0][1].tobytes() == runs[1][1].tobytes()
    for name in ("offsets", "first", "bytes"):
        assert getattr(runs[0][2], name).tobytes() == getattr(runs[1][2], name).tobytes(), name
    assert wres.n_distinct == 4 and wcodes[:3].tolist() == [2, 3, 0] and wres.n_matched == 46667


def test_chains_that_wrap(dev, xtwin):
    """The weak hash with prior entries and rows in the same four chains, which wrap through slot 0."""
    values = tdc.weak_values()
    arrays = arrays_of(values[:150:2], spare=(230, 2000))
    wres, _, _ = check(dev, xtwin, column_of(values[::-1] + values[::3]), arrays, 75, flags=(WEAK, 0, WEAK | FROZEN), shift=5)
    assert wres.n_matched == 75 + 25
    arrays = arrays_of(values[:150], spare=(150, 2000))
    got = device_extend(dev, tdg.OnDevice(dev, column_of(values[150:])), arrays, 150, WEAK)
    assert got[0].n_distinct == 300 and got[0].max_probe >= 37


# ---- past the grids ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("items", [SCAN_CHUNK * B + 1, ROW_GRID + 1 + 300])
def test_past_the_scan_chunk_and_the_row_grid(dev, xtwin, items):
    """All-distinct short values, generated: P + R = 262 145 items reach the second chunk of the block-sum scan with P and R
    each below it; 1 048 577 + 300 the second trip of the grid.  Half of the rows match prior entries."""
    P = items // 2
    R = items - P
    col = tdg.numbered(R, start=P - R // 2)
    arrays = numbered_prior(P, spare=(R - R // 2, 7 * (R - R // 2)))
    wres, wcodes, _ = check(dev, xtwin, col, arrays, P, shift=items % 16, where=items)
    assert wres.code == 0 and wres.n_matched == R // 2 and wres.n_distinct == P + R - R // 2
    assert np.array_equal(wcodes[:R], np.arange(P - R // 2, P - R // 2 + R, dtype=np.int32))


# ---- capacities -------------------------------------------------------------------------------------------------------------

def test_capacities(dev, xtwin):
    """One entry short, one byte short, none (dict_capacity == P exactly), more than enough: MSJ_CAPACITY where it is
    clipped, the codes complete, the counts exact, nothing past the capacities and nothing of the prior part written.  After a
    clipped call the repeat into larger arrays with the same P equals the unclipped twin."""
    prior = [b"v%d" % k for k in range(0, 300, 3)]
    values = [b"v%d" % (k % 300) * (1 + k % 4) for k in range(2000)] + [bytes([66]) * 700, b"", None, bytes([66]) * 700]
    col = column_of(values)
    a = tdg.OnDevice(dev, col)
    P, base = len(prior), sum(map(len, prior))
    _, new, _, _ = txm.definition(prior, values)
    n_new, new_bytes = len(new), sum(map(len, new))
    full = None
    for spare in ((n_new, new_bytes), (n_new - 1, new_bytes), (n_new, new_bytes - 1), (0, 0), (0, new_bytes), (n_new, 0), (1, 1), (n_new + 3, new_bytes + 9),
                  (B, new_bytes)):
        for flags in (0, WEAK):
            arrays = arrays_of(prior, spare=spare)
            wres, _, left = check(dev, xtwin, col, arrays, P, flags=(flags,), shift=sum(spare) % 16, a=a, where=spare)
            assert wres.code == (MSJ_CAPACITY if spare[0] < n_new or spare[1] < new_bytes else 0)
            assert (wres.n_distinct, wres.dict_bytes) == (P + n_new, base + new_bytes)
            if spare == (n_new, new_bytes):
                full = left
            elif wres.code == MSJ_CAPACITY:
                grown = Arrays(left.offsets[:P + 1].tolist(), left.bytes[:base].tobytes(), P + n_new, base + new_bytes)
                res, _, again = device_extend(dev, a, grown, P, flags)
                assert res.code == 0 and again.same(full), spare


def test_prior_count_on_the_device(dev, xtwin):
    """P as a word on the device equal to, below and above dict_capacity.  With P above it, with base above
    dict_bytes_capacity, or with R above rows, nothing but the four result members is written."""
    prior = [b"k%d" % c for c in range(40)]
    values = [b"k%d" % (k % 57) if k % 5 else None for k in range(2 * B + 7)]
    col = column_of(values)
    a = tdg.OnDevice(dev, col)
    for cap, p_word in ((40, 40), (70, 40), (40, 17), (70, 0)):
        arrays = arrays_of(prior, dict_capacity=cap, spare=(0, 200))
        wres, _, _ = check(dev, xtwin, col, arrays, None, flags=(0, FROZEN), a=a, p_word=p_word, where=(cap, p_word))
        assert wres.n_prior == p_word and wres.n_distinct == p_word   # (the last form is the frozen one)
    for flags in (0, FROZEN):
        for kw, R, P in ((dict(p_word=41), col.rows, 41), (dict(p_word=1 << 40), col.rows, 1 << 40), (dict(p_word=40, n_rows=col.rows + 1), col.rows + 1, 40)):
            arrays = arrays_of(prior, dict_capacity=40, spare=(0, 200))
            res, codes, left = device_extend(dev, a, arrays, 0, flags, **kw)
            assert summary(res) == (MSJ_CAPACITY, flags, R, 0, 0, 0, P, 0) and res.max_probe == 0, kw
            assert left.same(arrays) and bool((codes.view(np.uint8) == FILL).all())
        short = Arrays([0, 1, 9], b"abcdefghi", 5, 8)  # base = 9 above dict_bytes_capacity = 8
        res, codes, left = device_extend(dev, a, short, 0, flags, p_word=2)
        assert summary(res) == (MSJ_CAPACITY, flags, col.rows, 0, 0, 0, 2, 0) and left.same(short) and bool((codes.view(np.uint8) == FILL).all())


# ---- damaged inputs ---------------------------------------------------------------------------------------------------------

def test_damaged_prior(dev, xtwin):
    """Descending and out-of-range prior offsets over more than one block of prior entries: those entries match nothing, the
    others do.  Duplicate prior entries: the lower code wins."""
    rng = np.random.default_rng(33)
    P = 2 * B + 30
    prior = [b"w%d" % (c % 200) for c in range(P)]     # (c and c + 200 are duplicates)
    good = arrays_of(prior, spare=(300, 3000))
    off = good.offsets[:P + 1].copy()
    for c in rng.integers(1, P, 50):
        off[c] = [0, good.dict_bytes_capacity + 1 + int(c), (1 << 64) - 1, int(off[c - 1]), int(rng.integers(0, int(off[P])))][int(c) % 5]
    bad = good.copy()
    bad.offsets[:P + 1] = off
    values = [b"w%d" % (k % 260) for k in range(3 * B)] + [b"", None]
    for arrays in (good, bad):
        wres, wcodes, _ = check(dev, xtwin, column_of(values), arrays, P, flags=(0, WEAK, FROZEN))
    entries = bad.entries(P)
    assert 0 < sum(e is None for e in entries) < P
    wres, wcodes, _ = check(dev, xtwin, column_of(values), good, P)
    assert wcodes[:260].tolist() == list(range(200)) + list(range(P, P + 60))


def test_hostile_rows(dev, xtwin):
    """tests/test_dictionary.py's hostile row offsets and valid bytes over more than one block, against prior entries."""
    rng = np.random.default_rng(13)
    values = [b"w%d" % (k % 23) for k in range(2 * B + 40)]
    col = column_of(values)
    off = col.offsets.copy()
    for k in rng.integers(1, off.size - 1, 60):
        off[k] = [0, int(col.data.size) + 1 + int(k), (1 << 64) - 1, int(off[k - 1]), int(rng.integers(0, col.data.size))][int(k) % 5]
    valid = col.valid.copy()
    valid[::9] = rng.integers(0, 256, valid[::9].size)
    bad = tdc.Column(off, valid, col.data.tobytes())
    arrays = arrays_of([b"w%d" % c for c in range(0, 23, 2)], spare=(600, 6000))
    wres, _, _ = check(dev, xtwin, bad, arrays, 12, flags=(0, WEAK, FROZEN))
    assert 0 < wres.n_values < bad.rows and 0 < wres.n_matched < wres.n_values


# ---- frozen -----------------------------------------------------------------------------------------------------------------

def test_frozen_then_unfrozen(dev, xtwin):
    """Codes -2 / -1 / >= 0, the three arrays untouched over their whole length, n_matched; the same column unfrozen
    afterwards into the same arrays gives the appended result."""
    prior = [b"red", b"green", b""]
    values = [(b"red", b"blue", None, b"", b"grey", b"green")[k % 6] for k in range(3 * B + 5)]
    col = column_of(values)
    a = tdg.OnDevice(dev, col)
    arrays = arrays_of(prior, spare=(4, 16))
    res, codes, left = device_extend(dev, a, arrays, 3, FROZEN, shift=6)
    assert left.same(arrays) and codes[:6].tolist() == [0, NO_ENTRY, -1, 2, NO_ENTRY, 1]
    assert (res.code, res.n_distinct, res.dict_bytes, res.n_matched, res.n_values) == (0, 3, 8, sum(v in prior for v in values), sum(v is not None for v in values))
    wres, wcodes, wleft = check(dev, xtwin, col, left, 3, a=a, shift=6)
    assert wres.n_distinct == 5 and wcodes[:6].tolist() == [0, 3, -1, 2, 4, 1] and wleft.bytes[8:16].tobytes() == b"bluegrey"


# ---- arguments --------------------------------------------------------------------------------------------------------------

def test_bad_arguments(dev):
    """Each is refused with nothing launched, in the header's order: the outputs keep what was in them."""
    import torch

    col = column_of([b"a", b"b", b"a"])
    a = tdg.OnDevice(dev, col)
    sent = torch.full((8,), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    codes = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=dev.device)
    d_off = torch.full((8,), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    d_first = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=dev.device)
    out = torch.full((32,), 0x5A, dtype=torch.uint8, device=dev.device)
    n_rows = torch.full((2,), 3, dtype=torch.int64, device=dev.device)
    n_prior = torch.full((2,), 0, dtype=torch.int64, device=dev.device)

    def call(**kw):
        p = dict(off=a.d_offsets.data_ptr(), val=a.d_valid.data_ptr(), rows=3, n_rows=n_rows.data_ptr(), data=a.d_bytes.data_ptr(), len=a.bytes_len,
                 P=0, n_prior=n_prior.data_ptr(), codes=codes.data_ptr(), d_off=d_off.data_ptr(), d_first=d_first.data_ptr(), cap=4,
                 out=out.data_ptr(), room=16, flags=0, res=sent.data_ptr())
        p.update(kw)
        return dev.lib.msj_dictionary_extend_device(dev.ctx, p["off"], p["val"], p["rows"], p["n_rows"], p["data"], p["len"], p["P"], p["n_prior"],
                                                    p["codes"], p["d_off"], p["d_first"], p["cap"], p["out"], p["room"], p["flags"], p["res"],
                                                    dev._stream())

    none = dict(d_off=None, d_first=None, cap=0, out=None, room=0)
    assert dev.lib.msj_dictionary_extend_device(None, None, None, 0, None, None, 0, 0, None, None, None, None, 0, None, 0, 0, sent.data_ptr(),
                                                None) == BAD_ARGUMENT
    for name in ("res", "off", "val", "codes", "data", "d_off", "d_first", "out"):
        assert call(**{name: None}) == BAD_ARGUMENT, name
    assert call(P=1, n_prior=None, **none) == BAD_ARGUMENT and call(**none) == BAD_ARGUMENT   # prior entries and no arrays
    assert call(flags=4) == BAD_ARGUMENT and call(flags=7) == BAD_ARGUMENT
    assert call(flags=2, n_prior=None, **none) == BAD_ARGUMENT   # frozen and no arrays
    for name, base, step in (("off", a.d_offsets, 4), ("n_rows", n_rows, 4), ("n_prior", n_prior, 4), ("d_off", d_off, 4), ("res", sent, 4),
                             ("codes", codes, 2), ("d_first", d_first, 1)):
        assert call(**{name: base.data_ptr() + step}) == BAD_ARGUMENT, name
    torch.cuda.synchronize()
    assert bool((sent == tvd.SENTINEL).all()) and bool((d_off == tvd.SENTINEL).all()) and bool((out == 0x5A).all())
    assert bool((codes == 0x5A5A5A5A).all()) and bool((d_first == 0x5A5A5A5A).all())
    ws = dev.lib.msj_dictionary_extend_workspace_bytes
    assert ws(0, 0) >= 4 * tdc.MIN_SLOTS and ws(600, 400) >= ws(0, 0) + 12 * 1000 and ws(1 << 19, 1 << 19) >= 12 * (1 << 20) + 4 * (2 << 20)
    # an unaligned d_dict_bytes; then the same arrays as the prior dictionary, P by the argument; the layout-only form
    assert call(out=out.data_ptr() + 3, room=8, n_rows=None) == 0
    torch.cuda.synchronize()
    assert out.cpu().numpy()[3:6].tobytes() == b"ab\x5a" and codes.cpu().numpy()[:4].tolist() == [0, 1, 0, 0x5A5A5A5A]
    assert d_off.cpu().numpy()[:3].tolist() == [0, 1, 2] and d_first.cpu().numpy()[:3].tolist() == [0, 1, 0x5A5A5A5A]
    assert sent.cpu().numpy().tolist() == [0, 3, 3, 2, 2, sent.cpu().numpy()[5], 0, 0]
    assert call(out=out.data_ptr() + 3, room=8, P=1, n_prior=None) == 0
    torch.cuda.synchronize()
    assert codes.cpu().numpy()[:4].tolist() == [0, 1, 0, 0x5A5A5A5A] and sent.cpu().numpy()[[0, 1, 2, 3, 4, 6, 7]].tolist() == [0, 3, 3, 2, 2, 1, 2]
    assert call(n_prior=None, flags=1, **none) == 0
    torch.cuda.synchronize()
    assert sent.cpu().numpy()[[0, 1, 2, 3, 4, 6, 7]].tolist() == [1 << 32, 3, 3, 2, 2, 0, 0]   # code 0, flags 1


# ---- end to end -------------------------------------------------------------------------------------------------------------

def test_document_stream_with_a_running_dictionary(dev):
    """DocumentStream(select=[...]) over at least three windows with RunningDictionary, against dict.setdefault and
    json.loads over the WHOLE file: Window.categories (one value written with an escape in a later window),
    ListColumn.categories and MapColumn.key_categories; the sum of the windows' counts(); stats by status, merged over the
    windows by the header's rule; a dictionary that starts with room for 2 entries and 8 bytes and grows more than once;
    frozen=True against the dictionary of the first window only."""
    import torch
    from mojo_simdjson_amd.document_stream import DictionaryColumn, DocumentStream, RunningDictionary

    status = ["active", "suspended", "closed", "", "actíve"]
    docs = [{"n": k * 7 - 300, "status": status[(k * k) % 5] if k % 9 else "late-%d" % (k // 40), "tags": ["t%d" % (k % 4), k, "t%d" % (k // 25)],
             "attrs": {"color": k % 3, "n%d" % (k // 20): k}} for k in range(170)]
    docs[7] = {"n": "seven", "status": 5, "tags": 5}
    docs[11] = {"status": "closed"}
    docs[140] = {"n": 1 << 40, "status": "active"}   # (written with an escape below: the same value)
    lines = [json.dumps(d, ensure_ascii=False).encode() for d in docs]
    lines[140] = b'{"n":1099511627776,"status":"act\\u0069ve"}'
    data = b"\n".join(lines) + b"\n"
    text = lambda v: v.encode() if isinstance(v, str) else None

    class Whole:
        """dict.setdefault over the whole file, window by window"""

        def __init__(self):
            self.seen, self.counts = {}, []

        def window(self, values):
            prior = len(self.seen)
            codes = [self.seen.setdefault(v, len(self.seen)) if v is not None else -1 for v in values]
            self.counts += [0] * (len(self.seen) - len(self.counts))
            for c in codes:
                if c >= 0:
                    self.counts[c] += 1
            first = [codes.index(c) if c >= prior else -1 for c in range(len(self.seen))]
            return codes, first

    def agree(cats, whole, values, rd, what):
        assert isinstance(cats, DictionaryColumn) and cats.codes.dtype == torch.int32 and cats.codes.is_cuda and cats.bytes.is_cuda, what
        codes, first = whole.window([text(v) for v in values])
        assert cats.codes.cpu().tolist() == codes and cats.first.cpu().tolist() == first, what
        assert cats.values() == [v.decode() for v in whole.seen] == rd.values() and rd.n_distinct == cats.n_distinct == len(whole.seen), what
        return cats.counts().cpu().tolist()

    rds = {name: RunningDictionary(dev, dict_capacity=2, bytes_capacity=8) for name in ("status", "tags", "keys", "by")}
    wholes = {name: Whole() for name in ("status", "tags", "keys")}
    sums = {name: [] for name in wholes}
    grew = {name: [(rd.dict_capacity, rd.bytes_capacity)] for name, rd in rds.items()}
    merged, frozen_rd, frozen_want = {}, RunningDictionary(dev), None
    seen = windows = 0
    for win in DocumentStream(dev, tvd.upload(dev, data), len(data), window=4096, select=["/status", "/n", "/tags", "/attrs"]):
        D = win.n_documents
        mine = docs[seen:seen + D]
        per_window = {"status": agree(win.categories("/status", dictionary=rds["status"]), wholes["status"], [d.get("status") for d in mine],
                                      rds["status"], "status"),
                      "tags": agree(win.elements("/tags").categories(dictionary=rds["tags"]), wholes["tags"],
                                    [x for d in mine if isinstance(d.get("tags"), list) for x in d["tags"]], rds["tags"], "tags"),
                      "keys": agree(win.entries("/attrs").key_categories(dictionary=rds["keys"]), wholes["keys"],
                                    [key for d in mine for key in d.get("attrs", {})], rds["keys"], "keys")}
        for name, counts in per_window.items():
            sums[name] = [x + y for x, y in zip(sums[name] + [0] * (len(counts) - len(sums[name])), counts)]   # padded to n_distinct
        for name, rd in rds.items():
            grew[name].append((rd.dict_capacity, rd.bytes_capacity))
        # stats by status against the running dictionary: record g of every window is the same value
        stats = win.stats(["/n"], by="/status", dictionary=rds["by"])
        assert stats.n_groups == rds["by"].n_distinct and stats.keys.values() == rds["by"].values()
        for g, row in enumerate(stats.to_python()):
            m = merged.setdefault(g, {"key": row["key"], "n_rows": 0, "n_values": 0, "sum": 0, "min": None, "max": None})
            r = row["/n"]
            assert m["key"] == row["key"]
            m["n_rows"] += r["n_rows"]
            m["n_values"] += r["n_values"]
            if r["n_values"]:
                m["sum"] += r["sum"]
                m["min"] = r["min"] if m["min"] is None else min(m["min"], r["min"])
                m["max"] = r["max"] if m["max"] is None else max(m["max"], r["max"])
        # frozen against the dictionary of the first window only
        if windows == 0:
            first_window = frozen_rd.encode(win.strings("/status"))
            frozen_want = {v: c for c, v in enumerate(first_window.values())}
        else:
            cats = win.categories("/status", dictionary=frozen_rd, frozen=True)
            want = [-1 if not isinstance(d.get("status"), str) else frozen_want.get(d["status"], NO_ENTRY) for d in mine]
            assert cats.codes.cpu().tolist() == want and frozen_rd.n_distinct == len(frozen_want) == cats.n_distinct
            assert cats.first.cpu().tolist() == [-1] * len(frozen_want)
        seen += D
        windows += 1
    assert windows >= 3 and seen == len(docs)
    for name, whole in wholes.items():
        assert sums[name] == whole.counts and sum(whole.counts) > 100, name
    assert b"late-3" in wholes["status"].seen and "late-3" not in frozen_want   # (a value the frozen dictionary met as -2)
    assert len(set(grew["status"])) > 2 and len(set(grew["tags"])) > 2   # grew more than once
    assert list(wholes["status"].seen).count(b"active") == 1 and docs[140]["status"] == "active"
    want = {}
    for d in docs:
        s = d.get("status")
        if not isinstance(s, str):
            continue
        m = want.setdefault(s, {"key": s, "n_rows": 0, "n_values": 0, "sum": 0, "min": None, "max": None})
        m["n_rows"] += 1
        if isinstance(d.get("n"), int):
            n = d["n"]
            m["n_values"] += 1
            m["sum"] += n
            m["min"] = n if m["min"] is None else min(m["min"], n)
            m["max"] = n if m["max"] is None else max(m["max"], n)
    assert [merged[g] for g in range(len(merged))] == list(want.values())
