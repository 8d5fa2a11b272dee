"""An object's members as a map column on the device (msj_object_entries_device, csrc/object_entries_kernel.hip).

Expected values come from the host twin of the same arithmetic (tests/object_entries_math_host.cpp), which
tests/test_object_entries_math.py holds against the definition written in Python.  Device output is compared with the twin
over the WHOLE d_offsets, d_valid, d_keys and d_values arrays and the three results (every array starts from the same fill,
with 64 bytes of canary behind its capacity, so a store the twin does not make shows).  Inputs come both ways in: the oracles'
arrays and the twins' records, uploaded, and the real chain (shard, stage2_prep, documents, number_values,
validate_documents, select_documents, array_column, select_elements), whose device results the call reads.

The kernel constants the shapes lean on: a block of items_count / items_emit is 1 024 tokens (csrc/tape_block.h: kBlock), its
halo the ONE token behind it; a block of rows of the kernels over rows (csrc/rows_block.h) is 256 rows, and they sweep 1 024
of them per trip; rows_ranks takes 1 024 block sums of rows per chunk and items_scan 1 024 block counts of tokens.
"""
import json

import numpy as np
import pytest

from tests import helpers
from tests import test_array_column_math as tac
from tests import test_array_elements as tael
from tests import test_array_elements_math as tae
from tests import test_number_math as tnm
from tests import test_object_entries_math as tom
from tests import test_select_documents as tsd
from tests import test_select_elements_math as tse
from tests import test_select_math as tsm
from tests import test_string_column_math as tcm
from tests import test_tape_documents as ttd
from tests import test_tape_documents_math as tdk
from tests import test_validate_documents as tvd
from tests import test_validate_documents_math as tdm

pytestmark = pytest.mark.gpu

BLOCK = 1024                # tokens per workgroup of items_count / items_emit
ROW_BLOCK = 256             # rows per block of rows
SWEEP = 1024 * ROW_BLOCK    # rows one trip of the kernels over rows covers, and one chunk of rows_ranks
SCAN_CHUNK = 1024 * BLOCK   # tokens whose block counts items_scan takes in one round
MSJ_CAPACITY, BAD_ARGUMENT = 1, -1


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
def env(dev):
    e = tael.Env(dev)
    e.twins.o = tom.load_twin()
    return e


def device_maps(a, d_rows, d_rows_sel, want, numbers=True, numbers_result=True, numbers_capacity=None):
    """msj_object_entries_device over the arrays `a` with the twin's capacities, its arrays filled like the twin's with their
    canaries -> (tom.Maps, d_keys, d_values, d_keys_select, d_values_select)"""
    import torch
    from mojo_simdjson_amd import _lib

    dev = a.dev
    layout_only = want.keys is None
    offsets, valid, keys = tac.filled(want.capacity, want.entries_capacity, layout_only)
    up = lambda x: torch.from_numpy(x.view(np.int64).reshape(-1, 2)).to(dev.device)
    d_off = torch.from_numpy(offsets.view(np.int64)).to(dev.device)
    d_valid = torch.from_numpy(valid).to(dev.device)
    d_keys, d_values = (None, None) if layout_only else (up(keys), up(keys.copy()))
    d_ksel, d_vsel, d_res = (torch.full((48,), 0x5A, dtype=torch.uint8, device=dev.device) for _ in range(3))
    ncap = (a.ncap if numbers_capacity is None else numbers_capacity) if numbers else 0
    dev.object_entries(a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end, a.d_flags, d_rows, d_rows_sel, d_numbers=a.d_numbers if numbers else None,
                       numbers_capacity=ncap, d_numbers_result=a.d_num if numbers_result else None, d_offsets=d_off, d_valid=d_valid,
                       d_keys=d_keys, d_values=d_values, capacity=want.capacity, entries_capacity=want.entries_capacity, entries=not layout_only,
                       d_result=d_res, d_keys_select=d_ksel, d_values_select=d_vsel, sync=False)
    res = _lib.MsjObjectEntriesResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
    ksel, vsel = (_lib.MsjSelectDocumentsResult.from_buffer_copy(t.cpu().numpy().tobytes()) for t in (d_ksel, d_vsel))
    down = lambda t: np.ascontiguousarray(t.cpu().numpy()).view(tsm.FIELD_DTYPE).reshape(-1) if t is not None else None
    got = tom.Maps(res, ksel, vsel, d_off.cpu().numpy().view(np.uint64), d_valid.cpu().numpy(), down(d_keys), down(d_values), want.capacity,
                   want.entries_capacity)
    return got, d_keys, d_values, d_ksel, d_vsel


def same(got, want, where=None):
    """The device's results and every array are the twin's, fill and canary included"""
    assert got.summary() == want.summary(), (where, got.summary(), want.summary())
    for name in ("offsets", "valid", "keys", "values"):
        a, b = getattr(got, name), getattr(want, name)
        if b is None:
            assert a is None
            continue
        if name in ("keys", "values"):
            a, b = a.view(np.uint8).reshape(-1, 16), b.view(np.uint8).reshape(-1, 16)
            bad = np.nonzero((a != b).any(axis=1))[0]
        else:
            bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (where, name, int(bad[0]), a[bad[:3]].tolist(), b[bad[:3]].tolist(), bad.size)


class Case:
    """One window both ways: the oracles' arrays and the twins' rows of one source -- ("doc", pointer): a path's column, the
    rows are the documents; ("list", pointer): the element records of the list there; ("sub", pointer, sub): what `sub` finds
    in them --; on the device either all of that uploaded, or the real chain with the real select, array-column and
    select-elements calls."""

    def __init__(self, env, data, source, chain=False, verdicts=False, is_final=True, w=None):
        self.env, self.chain = env, chain
        self.w = w = tdm.WindowArrays(env.oracle, env.nm, data, is_final=is_final) if w is None else w
        self.verdict_rows = tdm.twin_documents(env.twins.v, w, 100)[0] if verdicts else None
        self.rows, self.rsel = tom.rows_of(env.twins, w, source, verdicts=self.verdict_rows)
        if chain:
            self.a = a = tsd.FromChain(env.dev, data, is_final, verdicts)
            assert a.n == w.n
            d_sel, d_cols = env.dev.select_documents(
                env.paths([source[1]]), a.d_buf, a.length, a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end, a.d_flags, a.d_first, a.d_docs,
                d_numbers=a.d_numbers, numbers_capacity=a.ncap, d_numbers_result=a.d_num, d_verdicts=a.d_verdicts, capacity=w.D + 3, sync=False)
            self.d_rows, self.d_rows_sel = d_cols[0], d_sel
            if source[0] != "doc":
                _, _, _, self.d_rows, self.d_rows_sel = env.dev.array_column(
                    a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end, a.d_flags, a.d_first, a.d_docs, d_cols, 0, d_sel, d_numbers=a.d_numbers,
                    numbers_capacity=a.ncap, d_numbers_result=a.d_num, elements_capacity=self.rows.size, sync=False)
            if source[0] == "sub":
                self.d_rows_sel, d_fields = env.dev.select_elements(
                    env.paths([source[2]]), a.d_buf, a.length, a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end, a.d_flags, self.d_rows,
                    self.d_rows_sel, d_numbers=a.d_numbers, numbers_capacity=a.ncap, d_numbers_result=a.d_num, capacity=self.rows.size, sync=False)
                self.d_rows = d_fields[0]
        else:
            self.a = tsd.Uploaded(env.dev, w, self.verdict_rows)
            self.d_rows, self.d_rows_sel = tael.upload_rows(env.dev, self.rows, self.rsel)

    def use(self, rows, rows_select=None):
        """Other records than the window's own (uploaded)"""
        self.rows = np.ascontiguousarray(rows)
        self.rsel = tse.rows_result(self.rows.size) if rows_select is None else rows_select
        self.d_rows, self.d_rows_sel = tael.upload_rows(self.env.dev, self.rows, self.rsel)
        return self

    def check(self, where=None, forms=(True, False), **kw):
        """The call on the device against the twin, in the layout-only form and with the records -> the twin's Maps"""
        for layout_only in forms:
            want = tom.twin_maps(self.env.twins.o, self.w, self.rows, self.rsel, layout_only=layout_only, **kw)
            dkw = {k: v for k, v in kw.items() if k in ("numbers", "numbers_result", "numbers_capacity")}
            got, self.d_keys, self.d_values, self.d_ksel, self.d_vsel = device_maps(self.a, self.d_rows, self.d_rows_sel, want, **dkw)
            same(got, want, (where, self.chain, layout_only, kw))
        return want

    def deeper(self, want):
        """Source 4: the call over its own values, where they lie on the device -> this Case with them as the rows"""
        self.rows, self.rsel = tom.next_level(want)
        self.d_rows, self.d_rows_sel = self.d_values, self.d_vsel
        return self


def both_ways(env, texts, source, verdicts=False, where=None, sep=b"\n", levels=1):
    """A window of documents both ways in, against the twin and the definition, `levels` deep through the call's own values
    -> (Case, the first level's Maps)"""
    data = tdk.join(texts, sep)
    for chain in (False, True):
        c = Case(env, data, source, chain, verdicts=verdicts)
        assert c.w.D == len(texts)
        values = tom.definition_rows(texts, source, [code for code, _ in c.verdict_rows] if verdicts else None)
        first = None
        for level in range(levels):
            want = c.check(where=(where, level))
            tom.check_against_definition(c.w, want, values)
            first = first or want
            c.deeper(want)
            values = tom.values_of(values)
    return c, first


def test_pins_and_corpus(env):
    """The pins of the CPU test, documents with a verdict code and a seeded corpus, for the four row sources -- the document
    column, list elements, a select-elements path and the call's own values two levels down: both ways in, against the twin
    and the definition."""
    c, want = both_ways(env, tom.PIN_TEXTS, ("doc", "/m"), levels=2)
    assert (want.res.n_objects, want.res.n_other, want.res.n_rows) == (10, 2, 13)
    bad = [b'{"m":{"a":1},"l":[{"b":2}]}', b'{"m":{"a":tru},"l":[{"b":2}]}', b'{"m":{"c":3,"d":4},"l":[]}', b'{"m":{"e":5},,"l":[{"x":1}]}',
           b'{"m":{},"l":[{"f":6},{"g":7,"h":8}]}']
    _, want = both_ways(env, bad, ("doc", "/m"), verdicts=True)
    assert want.offsets[:6].tolist() == [0, 1, 1, 3, 3, 3]
    _, want = both_ways(env, bad, ("list", "/l"), verdicts=True)
    assert want.offsets[:4].tolist() == [0, 1, 2, 4]
    texts = tom.seeded_documents(6100, 100)
    for j, source in enumerate(tom.SOURCES):
        c, want = both_ways(env, texts, source, where=source, sep=(b"\n", b" ", b"\r\n", b"", b"\n")[j], levels=3)
        assert c.w.n > 3 * BLOCK and want.res.n_rows >= 100


def keys_per_row(got):
    return tom.keys_per_row(got)


def test_halo_behind_the_block(env):
    """A first run of filler documents shifts the phase: the key of an entry sits at token offsets 1 020 .. 1 027 of the grid,
    so the key, its ':' and its value each land on either side of a block border, and the ':' of the block's last token
    comes from the halo."""
    doc = b'{"m":{"k":"v","q":[1],"z":{},"e":2}}'   # the row at f + 3; its keys at f + 4, f + 8, f + 14, f + 19
    for f in range(BLOCK - 8, BLOCK):
        head, k = tvd.filler(f, f % 2 == 0)
        tail, _ = tvd.filler(30, f % 2 == 1)
        c = Case(env, head + b"\n" + doc + b" " + tail + b"\n", ("doc", "/m"), chain=f % 2 == 1)
        assert int(c.w.first[k]) == f and c.rows["token"][k] == f + 3
        want = c.check(where=f)
        assert [t for t in keys_per_row(want) if t is not None] == [[f + 4, f + 8, f + 14, f + 19]]
    # (f = 1019: the key is token 1023, its ':' the halo, its value in the next block)


def test_keys_at_the_end_of_a_cut_window(env):
    """The last, short block of a non-final window: a key as token n - 4 .. n - 1.  The real chain leaves the unclosed object
    without a partner (no entry at all); uploaded, with the partner moved to the window's last token, the keys whose value
    lies in front of it are entries and the last ones are not -- nothing is read at or past n."""
    for lead in (7, BLOCK - 9, BLOCK - 3):
        head, _ = tvd.filler(lead, True)
        for k, cut in enumerate((b'{"a":1,"b":2,"c":3,', b'{"a":1,"b":2,"c":3', b'{"a":1,"b":2,"c":', b'{"a":1,"b":2,"c"')):
            data = head + b"\n" + cut
            w = tdm.WindowArrays(env.oracle, env.nm, data, is_final=False)
            n = w.n
            assert w.typ[n - 4 + k] == ord('"') and w.typ[lead] == ord("{") and n == lead + 13 - k
            chained = Case(env, data, ("doc", ""), chain=True, is_final=False, w=w).use(tom.record(lead)).check(where=(lead, k, "chain"))
            assert keys_per_row(chained) == [None] and chained.res.n_other == 1
            w.match = w.match.copy()
            w.match[lead] = n - 1
            moved = Case(env, data, ("doc", ""), is_final=False, w=w).use(tom.record(lead)).check(where=(lead, k, "moved"))
            assert keys_per_row(moved) == [[lead + 1, lead + 5] + ([lead + 9] if k == 0 else [])]


def test_rows_across_a_block_of_rows(env):
    """items[*].dims with R = 255, 256, 257: structs with and without dims -- live and coded records (20, and 17 for items
    that are no objects) -- mixed across the border of a block of 256 rows."""
    item = lambda j: (b'{"dims":{"w":%d,"h":[%d]}}' % (j, j), b'{"sku":%d}' % j, b"%d" % j, b'{"dims":{}}', b'{"dims":7}')[j % 5]
    for R in (255, 256, 257):
        texts = [b'{"items":[' + b",".join(item(j) for j in range(250)) + b"]}", b'{"items":[' + b",".join(item(j + 3) for j in range(R - 250)) + b"]}"]
        for chain in (False, True):
            c = Case(env, tdk.join(texts, b"\n"), ("sub", "/items", "/dims"), chain=chain)
            assert c.rows.size == R and sorted(set(c.rows["code"][248:R].tolist())) == [0, 17, 20]
            want = c.check(where=(R, chain))
            assert want.res.n_rows == R and want.res.n_other == sum(1 for j in list(range(250)) + list(range(3, R - 247)) if j % 5 == 4)
            assert want.res.n_entries == 2 * sum(1 for j in list(range(250)) + list(range(3, R - 247)) if j % 5 == 0)


def test_more_rows_than_one_sweep_and_a_second_scan_chunk(env):
    """263 000 elements {"k":j} and {} in one array -- the kernels over rows take their second trip and rows_ranks its second
    chunk of block sums -- in a window of more than 1 048 576 tokens, which gives items_scan its second chunk."""
    R = 263000
    data = b"[" + b",".join(b'{"k":%d}' % (j % 7) if j % 25 else b"{}" for j in range(R)) + b"]\n"
    c = Case(env, data, ("list", ""), chain=True)
    assert c.rows.size == R > SWEEP and c.w.n > SCAN_CHUNK
    want = c.check(where="sweep", forms=(False,))
    full = np.arange(R) % 25 != 0
    assert (want.res.code, want.res.n_rows, want.res.n_objects, want.res.n_entries) == (0, R, R, int(full.sum()))
    assert np.array_equal(want.offsets[:R + 1], np.concatenate([[0], np.cumsum(full)]).astype(np.uint64))
    assert want.values[:6]["bits"].tolist() == [1, 2, 3, 4, 5, 6]


def test_a_block_inside_one_row_and_blocks_no_row_reaches(env):
    """One object of 2 100 entries -- its middle blocks lie inside ONE row -- with nested objects whose members are not
    counted, short rows on either side; and whole blocks of {"x":1} that belong to no row, in front of the first row and
    between two rows: the early exits, and the rows behind them exact."""
    big = b"{" + b",".join(b'"k%d":{"in":%d}' % (j, j) if j % 50 == 0 else b'"k%d":%d' % (j, j) for j in range(2100)) + b"}"
    texts = [b'{"m":{"a":1}}'] * 3 + [b'{"m":' + big + b"}", b'{"m":{"b":2,"c":3}}']
    noise = b"[" + b",".join([b'{"x":1}'] * 400) + b"]"    # 2 801 tokens: whole blocks of candidates without a row
    quiet = [b'{"other":' + noise + b"}", b'{"m":{"a":1},"pad":' + noise + b',"d":{"e":5}}', b'{"m":{"b":2,"c":3}}', b'{"pad":' + noise + b"}",
             b'{"m":{"d":4}}']
    for chain in (False, True):
        c = Case(env, tdk.join(texts, b"\n"), ("doc", "/m"), chain=chain)
        want = c.check(where=("big", chain))
        t = c.rows["token"].tolist()
        assert (t[4] - 1) // BLOCK - t[3] // BLOCK >= 3 and want.offsets[:6].tolist() == [0, 1, 2, 3, 2103, 2105]
        c = Case(env, tdk.join(quiet, b"\n"), ("doc", "/m"), chain=chain)
        t = c.rows["token"].tolist()
        assert t[0] == 0xFFFFFFFF and t[1] // BLOCK >= 2 and t[2] // BLOCK - t[1] // BLOCK >= 2 and t[4] // BLOCK - t[2] // BLOCK >= 2
        want = c.check(where=("quiet", chain))
        assert want.offsets[:6].tolist() == [0, 0, 1, 3, 3, 4] and want.values[:4]["bits"].tolist() == [1, 2, 3, 4]


def test_capacities_and_stops(env):
    """capacity = R - 1; entries_capacity exact, n_entries - 1 and 1 (MSJ_CAPACITY, the offsets complete, the canaries intact)
    and the layout-only form; R == 0; n == 0; d_rows_select with a code; a swapped and an equal live pair, also across a
    block of rows: only the results are written."""
    texts = [b'{"m":{"a":%d,"b":"s","c":[1],"d":{"k":2}},"x":{"y":1}}' % k if k % 3 else b'{"m":7}' for k in range(300)]
    data = tdk.join(texts, b"\n")
    R, total = 300, 800
    for chain in (False, True):
        c = Case(env, data, ("doc", "/m"), chain=chain)
        for kw in (dict(entries_capacity=total), dict(entries_capacity=total - 1), dict(entries_capacity=1), dict(entries_capacity=0),
                   dict(capacity=R + 300, entries_capacity=total + 100)):
            want = c.check(where=(chain, kw), forms=(False,), **kw)
            assert want.res.n_entries == total and want.res.code == (MSJ_CAPACITY if kw["entries_capacity"] < total else 0)
            assert want.untouched(R, min(kw["entries_capacity"], total))
        assert (want.res.n_objects, want.res.n_other) == (200, 100)
        layout = c.check(where=chain, forms=(True,))
        assert layout.res.code == 0 and layout.res.n_entries == total
        for cap in (R - 1, 0, 1):
            over = c.check(where=(chain, cap), capacity=cap, entries_capacity=total)
            assert over.summary() == tom.stop_summary(MSJ_CAPACITY, R) and over.untouched(-1, 0)
    c = Case(env, data, ("doc", "/m"))
    rows = c.rows.copy()
    for code in (9, -1, MSJ_CAPACITY):
        got = c.use(rows, tse.rows_result(R, code)).check(capacity=R, entries_capacity=total)
        assert got.summary() == tom.stop_summary(code) and got.untouched(-1, 0)
    for chain in (False, True):   # R == 0: a list without an element; n == 0: no token
        none = Case(env, b'{"l":[]}\n{"other":[{"a":1}]}\n', ("list", "/l"), chain=chain).check(capacity=3, entries_capacity=2)
        assert none.summary() == tom.stop_summary(0) and none.offsets[0] == 0 and none.untouched(0, 0)
        c0 = Case(env, b"  \n ", ("doc", "/m"), chain=chain, is_final=False)
        assert c0.w.n == 0 and c0.check(capacity=2, entries_capacity=2).summary() == tom.stop_summary(0)
    lost = c0.use(rows[1:5]).check(capacity=5, entries_capacity=2)   # records of another window over no token at all
    assert lost.summary()[:7] == (0, 0, 4, 0, 0, 4, 0) and lost.offsets[:5].tolist() == [0] * 5 and lost.untouched(4, 0)
    # the order: a swapped and an equal pair of live rows
    w = tom.hostile_window(env.oracle, env.nm)
    c = Case(env, w.data, ("doc", ""), w=w)
    rec, coded = tom.record, tom.coded
    good = [rec(tom.FIRST), rec(tom.INNER), rec(tom.OTHER), rec(tom.LAST)]
    for order in ([1, 0, 2, 3], [0, 1, 3, 2], [0, 1, 2, 2], [3, 0, 1, 2]):
        for gap in ([], [coded(20)], [coded(17)] * 300):
            rows = []
            for j in order:
                rows += [good[j]] + gap
            got = c.use(np.concatenate(gap + rows)).check(where=(order, len(gap)), entries_capacity=8)
            assert got.summary() == tom.stop_summary(BAD_ARGUMENT, len(gap) * 5 + 4) and got.untouched(-1, 0)


def test_numbers(env):
    """Number values with their records, with d_numbers NULL, with d_numbers_result NULL and with a numbers_capacity that ends
    inside the window: the bits, or MSJ_FIELD_NO_BITS counted in the result and the values' select result -- never in the
    keys' --, and only for the records written."""
    texts = [b'{"m":{"a":%d,"b":%d.5,"c":-1e%d,"d":"x","e":[%d]}}' % (k, k, k % 30, k) for k in range(400)]   # 5 entries per line, 3 number values; 4 number tokens
    for chain in (False, True):
        c = Case(env, tdk.join(texts, b"\n"), ("doc", "/m"), chain=chain)
        full = c.check(where=chain)
        assert full.res.n_entries == 2000 and full.res.n_no_bits == 0 and full.values[5]["bits"] == 1
        for kw, nobits in ((dict(numbers=False), 1200), (dict(numbers_result=False), 1200), (dict(numbers_capacity=800), 600),
                           (dict(numbers_capacity=0), 1200)):
            part = c.check(where=(chain, kw), forms=(False,), **kw)
            assert (part.res.n_no_bits, part.vsel.n_no_bits, part.ksel.n_no_bits) == (nobits, nobits, 0), (kw, part.summary())
        clip = c.check(where=chain, forms=(False,), numbers=False, entries_capacity=700)
        assert clip.res.n_no_bits == 420 and clip.vsel.n_no_bits == 420 and clip.res.code == MSJ_CAPACITY


def test_hostile_records(env):
    """Uploaded: coded records between live ones across blocks of rows, records that lie, a row inside a row, a row whose own
    token is a key, tokens at or past n, partners moved, every token a row, malformed members: nothing faults, the output
    stays inside the canaries and the device follows the twin."""
    w = tom.hostile_window(env.oracle, env.nm)
    c = Case(env, w.data, ("doc", ""), w=w)
    rec, coded = tom.record, tom.coded
    good = [rec(tom.FIRST), rec(tom.INNER), rec(tom.OTHER), rec(tom.LAST)]
    rows = []
    for g in good:
        rows += [coded(17)] * 300 + [g]
    fine = c.use(np.concatenate(rows + [coded(20)] * 300)).check(where="gaps")
    assert [t for t in keys_per_row(fine) if t is not None] == [[4, 8], [11], [22], [25]] and fine.offsets[1204:1505].tolist() == [5] * 301
    lying = np.concatenate([rec(tom.OUTER, typ="["), rec(tom.FIRST), rec(5), rec(8), rec(tom.INNER, typ='"'), coded(17), rec(tom.OTHER + 1),
                            rec(w.n), rec(w.n + 7), rec(tom.NO_TOKEN)])
    want = c.use(lying).check(where="lying")
    assert keys_per_row(want) == [None, [4]] + [None] * 8
    own = c.use(np.concatenate([rec(tom.FIRST), rec(8)])).check(where="own")
    assert keys_per_row(own) == [[4, 8], None] and own.offsets[:3].tolist() == [0, 2, 2]
    nested = c.use(np.concatenate([rec(tom.OUTER), coded(20), rec(tom.FIRST)])).check(where="nested")
    assert keys_per_row(nested) == [[1], None, [4, 8]]
    for m in (w.n, w.n + 5, tdk.NO_PARTNER, tom.INNER, tom.INNER - 1, 0, w.n - 1, 14, 13):
        w.match = w.match.copy()
        w.match[tom.INNER] = m
        edited = Case(env, w.data, ("doc", ""), w=w).use(np.concatenate([rec(tom.FIRST), rec(tom.INNER), rec(tom.OTHER)])).check(where=m)
        assert keys_per_row(edited) == [[4, 8], [11] if m in (w.n - 1, 14) else ([] if m == 13 else None), [22]]
    text = tom.every_token_a_row()
    w = tdm.WindowArrays(env.oracle, env.nm, text, is_final=True)
    n = w.n
    for lo, hi, step in ((0, n, 1), (0, n, 2), (BLOCK - 1, 2 * BLOCK + 1, 1), (0, n + 5, 1)):
        rows = np.concatenate([rec(v) for v in range(lo, hi, step)])
        want = Case(env, text, ("doc", ""), w=w).use(rows).check(where=(lo, hi, step))
        assert want.res.n_objects == int((w.typ[lo:min(hi, n):step] == ord("{")).sum())
    for text, pins in tom.MALFORMED:
        w = tdm.WindowArrays(env.oracle, env.nm, text + b"\n", is_final=True)
        for chain in (False, True):
            bad = Case(env, text + b"\n", ("doc", ""), chain=chain, w=w).use(tom.malformed_rows(w)).check(where=(text, chain))
            assert bad.res.n_entries == len(pins)


def test_composition_on_the_device(env):
    """The new records as the rows of the next call, where they lie on the device: msj_string_column_device over the keys
    gives the JSON keys, escaped ones included; msj_array_elements_device and msj_select_elements_device over the values run
    unchanged and match their twins."""
    import torch

    dev = env.dev
    names = ["ab", "c\nd", "", "é\U0001F600", 'q"\\/', "plain" * 9]
    docs = [{"m": {names[(k + j) % 6] + str(j): [[k, j], {"sku": k, "tags": [names[j % 6]]}][j % 2] for j in range(k % 5)}} for k in range(200)]
    texts = [json.dumps(d, ensure_ascii=bool(k % 2)).encode() for k, d in enumerate(docs)]
    data = tdk.join(texts, b"\n")
    for chain in (False, True):
        c = Case(env, data, ("doc", "/m"), chain=chain)
        a = c.a
        want = c.check(where=chain)
        pairs = [(key, v) for d in docs for key, v in d["m"].items()]
        n = len(pairs)
        assert want.res.n_entries == n > 300
        # the keys as a string column
        col = tcm.twin_column(env.ctwin, data, want.keys[:n], n)
        offsets, valid, out = tcm.filled(n, col.bytes_capacity)
        res, d_off, d_valid, d_bytes = dev.string_column(a.d_buf, len(data), c.d_keys.unsqueeze(0), 0, c.d_ksel,
                                                         d_offsets=torch.from_numpy(offsets.view(np.int64)).to(dev.device),
                                                         d_valid=torch.from_numpy(valid).to(dev.device), d_bytes=torch.from_numpy(out).to(dev.device),
                                                         capacity=n, bytes_capacity=col.bytes_capacity)
        assert (res.code, res.n_rows, res.n_strings, res.total_bytes) == (0, n, n, col.res.total_bytes)
        assert np.array_equal(d_off.cpu().numpy().view(np.uint64), col.offsets) and np.array_equal(d_bytes.cpu().numpy(), col.data)
        assert col.rows() == [key.encode("utf-8") for key, _ in pairs]
        # the lists among the values: msj_array_elements_device over d_values / d_values_select
        lists = tae.twin_lists(env.twins.l, c.w, want.values[:n].copy(), want.vsel)
        got, _, _ = tael.device_lists(a, c.d_values, c.d_vsel, lists)
        tael.same(got, lists, (chain, "lists"))
        assert lists.res.n_arrays == sum(isinstance(v, list) for _, v in pairs) and lists.res.n_elements == 2 * lists.res.n_arrays
        # fields by path inside the values: msj_select_elements_device over them
        sel_want = tse.twin_elements(env.twins, c.w, ["/sku", "/tags"], want.values[:n], want.vsel)
        d_sel, d_fields = dev.select_elements(env.paths(["/sku", "/tags"]), a.d_buf, a.length, a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end,
                                              a.d_flags, c.d_values, c.d_vsel, d_numbers=a.d_numbers, numbers_capacity=a.ncap,
                                              d_numbers_result=a.d_num, capacity=n, sync=False)
        got_fields = np.ascontiguousarray(d_fields.cpu().numpy()).view(tsm.FIELD_DTYPE).reshape(2, -1)
        assert np.array_equal(got_fields[:, :n], np.stack([sel_want.column(0)[:n], sel_want.column(1)[:n]]))
        assert sel_want.res.n_found == 2 * sum(isinstance(v, dict) for _, v in pairs)


def test_bad_arguments_and_check_order(env):
    """Each NULL, off-grid and aliasing case is refused with nothing launched: the outputs keep what was in them.  Two faults
    at once: missing arrays are judged before the size, the size before outputs and alignment."""
    import torch

    dev = env.dev
    c = Case(env, b'{"m":{"a":1,"b":"s"}}\n{"m":{"c":2}}\n', ("doc", "/m"), chain=True)
    a = c.a
    mk = lambda shape: torch.full(shape, tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    sent, ksel, vsel, off, keys, vals = mk((6,)), mk((6,)), mk((6,)), mk((8,)), mk((8, 2)), mk((8, 2))
    val = torch.full((16,), 0x5A, dtype=torch.uint8, device=dev.device)
    tensors = dict(idx=a.d_idx, type=a.d_type, depth=a.d_depth, match=a.d_match, end=a.d_end, flags=a.d_flags, numbers=a.d_numbers, num=a.d_num,
                   rows=c.d_rows, sel=c.d_rows_sel, off=off, val=val, keys=keys, vals=vals, res=sent, ksel=ksel, vsel=vsel)

    def call(**kw):
        p = {k: t.data_ptr() for k, t in tensors.items()}
        p.update(ctx=dev.ctx, n=a.n, ncap=a.ncap, cap=2, room=8)
        p.update(kw)
        return dev.lib.msj_object_entries_device(p["ctx"], p["idx"], p["n"], p["type"], p["depth"], p["match"], p["end"], p["flags"], p["numbers"],
                                                 p["ncap"], p["num"], p["rows"], p["sel"], p["off"], p["val"], p["cap"], p["keys"], p["vals"],
                                                 p["room"], p["res"], p["ksel"], p["vsel"], dev._stream())

    assert call(n=1 << 31) == MSJ_CAPACITY
    for name in ("ctx", "res", "sel", "idx", "type", "depth", "match", "end", "flags", "rows", "off", "val", "keys", "vals", "numbers"):
        assert call(**{name: None}) == BAD_ARGUMENT, name
    assert call(keys=None, room=0) == BAD_ARGUMENT and call(vals=None, room=0) == BAD_ARGUMENT    # exactly one of the two
    ptr = lambda name: tensors[name].data_ptr()
    for kw in (dict(ksel=ptr("sel")), dict(vsel=ptr("sel")), dict(ksel=ptr("vsel")), dict(keys=ptr("rows")), dict(vals=ptr("rows")),
               dict(keys=ptr("vals"))):
        assert call(**kw) == BAD_ARGUMENT, kw
    for name, step in (("idx", 8), ("depth", 4), ("match", 8), ("end", 4), ("numbers", 8), ("rows", 8), ("keys", 8), ("vals", 8), ("type", 4),
                       ("flags", 1), ("num", 4), ("sel", 4), ("off", 4), ("res", 4), ("ksel", 4), ("vsel", 4)):
        assert call(**{name: ptr(name) + step}) == BAD_ARGUMENT, name
    assert call(type=None, n=1 << 31) == BAD_ARGUMENT
    assert call(n=1 << 31, idx=ptr("idx") + 4) == MSJ_CAPACITY
    assert call(keys=None, depth=ptr("depth") + 4) == BAD_ARGUMENT
    torch.cuda.synchronize()
    for t in (sent, ksel, vsel, off, keys, vals):
        assert bool((t == tvd.SENTINEL).all())
    assert bool((val == 0x5A).all()) and dev.lib.msj_object_entries_workspace_bytes(0, 0) > 0
    # an unaligned d_valid, no select results, no number records
    assert call(val=val.data_ptr() + 1, ksel=None, vsel=None, numbers=None, ncap=0, num=None) == 0
    torch.cuda.synchronize()
    t0 = int(c.rows["token"][0])
    assert sent.cpu().numpy().tolist() == [0, 2, 2, 3, 0, 2] and val.cpu().numpy()[1:3].tolist() == [1, 1] and off.cpu().numpy()[:3].tolist() == [0, 2, 3]
    assert keys.cpu().numpy()[:2, 1].tolist() == [t0 + 1 | ord('"') << 32, t0 + 5 | ord('"') << 32]
    assert vals.cpu().numpy()[:2, 1].tolist() == [t0 + 3 | ord("l") << 32 | 64 << 40, t0 + 7 | ord('"') << 32]
    assert bool((ksel == tvd.SENTINEL).all()) and bool((vsel == tvd.SENTINEL).all()) and bool((keys[3:] == tvd.SENTINEL).all())
    # the layout-only form, and no capacity at all with NULL arrays: R = 2 > 0 is MSJ_CAPACITY, in all three results
    assert call(keys=None, vals=None, room=0) == 0 and call(rows=None, off=None, val=None, cap=0, keys=None, vals=None, room=0) == 0
    torch.cuda.synchronize()
    assert sent.cpu().numpy().tolist() == [MSJ_CAPACITY, 2, 0, 0, 0, 0]
    assert ksel.cpu().numpy().tolist() == [MSJ_CAPACITY, 0, 1, 0, 0, 0] and vsel.cpu().numpy().tolist() == [MSJ_CAPACITY, 0, 1, 0, 0, 0]


def test_document_stream_maps(env):
    """A few hundred lines of NDJSON through windows of 4 096 bytes, DocumentStream(select=["/attrs", "/items", "/mm"]):
    Window.entries, ListColumn.entries, ElementFields.entries and MapColumn.keys / values / to_python equal json on every
    line, a map of maps through .values().entries() included; the buffers have to grow in every other window."""
    import torch
    from mojo_simdjson_amd.document_stream import DocumentStream, ListColumn, MapColumn

    dev = env.dev
    attrs = lambda k: {"k%d\n" % j if j % 3 else "é%d" % j: [j, "v%d" % k, j + 0.5, [j], {"in": j}][(k + j) % 5] for j in range(k % 6)}
    items = lambda k: [{"sku": j, "dims": {"w": k + j, "h\t": "x"}} if (k + j) % 4 else [{"sku": 1}, 7, {"dims": 5}][(k + j) % 3] for j in range(k % 4)]
    mm = lambda k: {"a%d" % j: {"b%d" % i: i + k for i in range(j)} if j % 3 else j for j in range(k % 5)}
    lines = [json.dumps({"id": k, "attrs": attrs(k) if k % 9 else "none", "items": items(k), "mm": mm(k), "pad": "p" * (k % 40)},
                        ensure_ascii=bool(k % 2)).encode() for k in range(300)]
    lines[100] = b'{"id":100,"attrs":{"a":tru},"items":[],"mm":{}}'
    lines[101] = b'{"id":101,"attrs":{"d":1,"d":2,"e":3},"items":[],"mm":{}}'
    data = b"\n".join(lines) + b"\n"
    docs = [None if k == 100 else json.loads(line, object_pairs_hook=lambda p: tom.plain(tom.Pairs(p))) for k, line in enumerate(lines)]
    as_map = lambda v: v if isinstance(v, dict) else None
    want_attrs = [as_map(d["attrs"]) if d else None for d in docs]
    want_items = [as_map(item) for d in docs if d for item in d["items"]]
    want_dims = [as_map(item.get("dims")) if isinstance(item, dict) else None for d in docs if d for item in d["items"]]
    want_inner = [as_map(v) for d in docs if d for v in d["mm"].values()]
    stream = DocumentStream(dev, tvd.upload(dev, data), len(data), window=4096, select=["/attrs", "/items", "/mm"])
    got_attrs, got_items, got_dims, got_inner, got_keys, got_nums, windows = [], [], [], [], [], [], 0
    for win in stream:
        m = win.entries("/attrs", entries_capacity=1 if windows % 2 else None)   # (1: the buffers have to grow)
        assert isinstance(m, MapColumn) and m.parent is None and m.window is win and m.offsets.shape == (win.n_documents + 1,)
        assert m.key_fields.shape == m.value_fields.shape == (m.n_entries, 2) and m.valid.dtype == torch.bool and m.key_fields.is_cuda
        got_attrs += m.to_python()
        k_off, k_bytes, k_valid = m.keys()
        ko, raw = k_off.cpu().tolist(), k_bytes.cpu().numpy().tobytes()
        assert bool(k_valid.all()) or m.n_entries == 0
        keys = [raw[ko[j]:ko[j + 1]].decode("utf-8") for j in range(m.n_entries)]
        off = m.offsets.cpu().tolist()
        got_keys += [keys[off[r]:off[r + 1]] for r in range(win.n_documents)]
        values = m.values()
        assert isinstance(values, ListColumn) and values.parent is m and values.offsets is m.offsets and values.n_elements == m.n_entries
        nums, ok = values.numbers(torch.float64)
        flat = [v if good else None for v, good in zip(nums.cpu().tolist(), ok.cpu().tolist())]
        got_nums += [flat[off[r]:off[r + 1]] for r in range(win.n_documents)]
        items_col = win.elements("/items")
        got_items += items_col.entries(entries_capacity=None if windows % 2 else 1).to_python()
        fields = items_col.select(["/dims"])
        dims = fields.entries("/dims")
        assert dims.parent is fields and dims.offsets.shape == (fields.n_elements + 1,)
        got_dims += dims.to_python()
        inner = win.entries("/mm").values().entries()       # a map of maps
        assert inner.parent.parent.parent is None
        got_inner += inner.to_python()
        windows += 1
    assert windows >= 6 and sum(len(m) for m in got_attrs if m) > 400 and sum(1 for m in got_dims if m) > 100
    assert got_attrs == want_attrs and got_attrs[101] == {"d": 1, "e": 3}
    assert got_items == want_items and got_dims == want_dims and got_inner == want_inner and sum(len(m) for m in got_inner if m) > 100
    lists = lambda k: [key for key, _ in json.loads(lines[k], object_pairs_hook=tom.Pairs)[1][1]] if want_attrs[k] is not None else []
    assert got_keys == [lists(k) for k in range(300)] and got_keys[101] == ["d", "d", "e"]
    is_num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
    pairs = lambda k: json.loads(lines[k], object_pairs_hook=tom.Pairs)[1][1] if want_attrs[k] is not None else []
    assert got_nums == [[float(v) if is_num(v) else None for _, v in pairs(k)] for k in range(300)]
