"""The arrays inside list rows as a list column on the device (msj_array_elements_device, csrc/array_elements_kernel.hip).

Expected values come from the host twin of the same arithmetic (tests/array_elements_math_host.cpp), which
tests/test_array_elements_math.py holds against the definition written in Python.  Device output is compared with the twin
over the WHOLE d_offsets, d_valid and d_elements arrays and the two results (every array starts from the same fill, with 64
bytes of canary behind its capacity, so a store the twin does not make shows).  Inputs come both ways in: the oracles' arrays
and the twins' records, uploaded, and the real chain (shard, stage2_prep, documents, number_values, validate_documents,
select_documents, array_column, select_elements), whose device results the call reads.

The kernel constants the shapes lean on: a block of items_count / items_emit (csrc/rows_block.h) is 1 024 tokens
(csrc/tape_block.h: kBlock); a block of rows of rows_live / rows_place is 256 rows, and the kernels over rows sweep 1 024 of
them per trip; rows_ranks takes 1 024 block sums of rows per chunk and items_scan 1 024 block counts of tokens.
"""
import json

import numpy as np
import pytest

from tests import helpers
from tests import test_array_column_math as tac
from tests import test_array_elements_math as tae
from tests import test_number_math as tnm
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
ROW_BLOCK = 256             # rows per block of rows of rows_live / rows_place
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
    return Env(dev)


class Env:
    """The device, the oracles and the twins, and the compiled paths of every pointer list used so far"""

    def __init__(self, dev):
        self.dev, self.oracle, self.nm = dev, helpers.load_oracle(), tnm.load_twin()
        self.twins, self.ctwin = tse.Twins(), tcm.load_twin()
        self.twins.l = tae.load_twin()
        self._paths = {}

    def paths(self, pointers):
        key = tuple(pointers)
        if key not in self._paths:
            self._paths[key] = self.dev.compile_paths(pointers)
        return self._paths[key]


def upload_rows(dev, rows, rows_select):
    """Records as d_rows of shape (rows + 1, 2) -- never an empty tensor -- and their select result"""
    padded = np.concatenate([np.ascontiguousarray(rows), np.zeros(1, dtype=tsm.FIELD_DTYPE)])
    return ttd.to_device(dev, padded).reshape(-1, 2), ttd.to_device(dev, np.frombuffer(bytes(rows_select), dtype=np.uint8))


def device_lists(a, d_rows, d_rows_sel, want, numbers=True, numbers_result=True, numbers_capacity=None):
    """msj_array_elements_device over the arrays `a` with the twin's capacities, its arrays filled like the twin's with their
    canaries -> (tac.Lists, d_elements, d_elements_select)"""
    import torch
    from mojo_simdjson_amd import _lib

    dev = a.dev
    offsets, valid, elements = tac.filled(want.capacity, want.elements_capacity, want.elements is None)
    d_off = torch.from_numpy(offsets.view(np.int64)).to(dev.device)
    d_valid = torch.from_numpy(valid).to(dev.device)
    d_el = torch.from_numpy(elements.view(np.int64).reshape(-1, 2)).to(dev.device) if elements is not None else None
    d_esel = torch.full((48,), 0x5A, dtype=torch.uint8, device=dev.device)
    d_res = torch.full((48,), 0x5A, dtype=torch.uint8, device=dev.device)
    ncap = (a.ncap if numbers_capacity is None else numbers_capacity) if numbers else 0
    dev.array_elements(a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end, a.d_flags, d_rows, d_rows_sel, d_numbers=a.d_numbers if numbers else None,
                       numbers_capacity=ncap, d_numbers_result=a.d_num if numbers_result else None, d_offsets=d_off, d_valid=d_valid,
                       d_elements=d_el, capacity=want.capacity, elements_capacity=want.elements_capacity, elements=elements is not None,
                       d_result=d_res, d_elements_select=d_esel, sync=False)
    res = _lib.MsjArrayColumnResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
    esel = _lib.MsjSelectDocumentsResult.from_buffer_copy(d_esel.cpu().numpy().tobytes())
    got = np.ascontiguousarray(d_el.cpu().numpy()).view(tsm.FIELD_DTYPE).reshape(-1) if elements is not None else None
    return tac.Lists(res, esel, d_off.cpu().numpy().view(np.uint64), d_valid.cpu().numpy(), got, want.capacity, want.elements_capacity), d_el, d_esel


def same(got, want, where=None):
    """The device's results and every array are the twin's, fill and canary included"""
    assert got.summary() == want.summary(), (where, got.summary(), want.summary())
    for name in ("offsets", "valid", "elements"):
        a, b = getattr(got, name), getattr(want, name)
        if b is None:
            assert a is None
            continue
        if name == "elements":
            a, b = a.view(np.uint8).reshape(-1, 16), b.view(np.uint8).reshape(-1, 16)
            bad = np.nonzero((a != b).any(axis=1))[0]
        else:
            bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (where, name, int(bad[0]), a[bad[:3]].tolist(), b[bad[:3]].tolist(), bad.size)


class Case:
    """One window both ways: the oracles' arrays and the twins' rows -- the element records of the list at `list_pointer`, or
    what `sub` finds in them --; on the device either all of that uploaded, or the real chain with the real select,
    array-column and select-elements calls."""

    def __init__(self, env, data, list_pointer, sub=None, chain=False, verdicts=False, is_final=True, w=None):
        self.env, self.chain = env, chain
        self.w = w = tdm.WindowArrays(env.oracle, env.nm, data, is_final=is_final) if w is None else w
        self.verdict_rows = tdm.twin_documents(env.twins.v, w, 100)[0] if verdicts else None
        self.rows, self.rsel = tae.parent_rows(env.twins, w, list_pointer, sub, verdicts=self.verdict_rows)
        if chain:
            self.a = a = tsd.FromChain(env.dev, data, is_final, verdicts)
            assert a.n == w.n
            d_sel, d_cols = env.dev.select_documents(
                env.paths([list_pointer]), a.d_buf, a.length, a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end, a.d_flags, a.d_first, a.d_docs,
                d_numbers=a.d_numbers, numbers_capacity=a.ncap, d_numbers_result=a.d_num, d_verdicts=a.d_verdicts, capacity=w.D + 3, sync=False)
            self.list_call = lambda room: env.dev.array_column(
                a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end, a.d_flags, a.d_first, a.d_docs, d_cols, 0, d_sel, d_numbers=a.d_numbers,
                numbers_capacity=a.ncap, d_numbers_result=a.d_num, elements_capacity=room, sync=False)
            _, _, _, self.d_rows, self.d_rows_sel = self.list_call(self.rows.size)
            if sub is not None:
                self.d_rows_sel, d_fields = env.dev.select_elements(
                    env.paths([sub]), a.d_buf, a.length, a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end, a.d_flags, self.d_rows,
                    self.d_rows_sel, d_numbers=a.d_numbers, numbers_capacity=a.ncap, d_numbers_result=a.d_num, capacity=self.rows.size, sync=False)
                self.d_rows = d_fields[0]
        else:
            self.a = tsd.Uploaded(env.dev, w, self.verdict_rows)
            self.d_rows, self.d_rows_sel = upload_rows(env.dev, self.rows, self.rsel)

    def use(self, rows, rows_select=None):
        """Other records than the window's own (uploaded)"""
        self.rows = np.ascontiguousarray(rows)
        self.rsel = tse.rows_result(self.rows.size) if rows_select is None else rows_select
        self.d_rows, self.d_rows_sel = upload_rows(self.env.dev, self.rows, self.rsel)
        return self

    def check(self, where=None, forms=(True, False), **kw):
        """The call on the device against the twin, in the layout-only form and with the elements -> the twin's Lists"""
        for layout_only in forms:
            want = tae.twin_lists(self.env.twins.l, self.w, self.rows, self.rsel, layout_only=layout_only, **kw)
            dkw = {k: v for k, v in kw.items() if k in ("numbers", "numbers_result", "numbers_capacity")}
            got, self.d_elements, self.d_esel = device_lists(self.a, self.d_rows, self.d_rows_sel, want, **dkw)
            same(got, want, (where, self.chain, layout_only, kw))
        return want


def both_ways(env, texts, list_pointer, sub=None, verdicts=False, where=None, sep=b"\n"):
    """A window of documents both ways in, against the twin and the definition -> (Case, the twin's Lists, the rows' values)"""
    data = tdk.join(texts, sep)
    for chain in (False, True):
        c = Case(env, data, list_pointer, sub, chain, verdicts=verdicts)
        assert c.w.D == len(texts)
        want = c.check(where=where)
    values = tae.definition(texts, list_pointer, sub, [code for code, _ in c.verdict_rows] if verdicts else None)
    tac.check_against_definition(c.w, want, values)
    return c, want, values


def test_pins_and_corpus(env):
    """The pins of the CPU test, documents with a verdict code and a seeded corpus, lists of lists and lists inside lists of
    structs: both ways in, against the twin and the definition."""
    c, want, _ = both_ways(env, tae.PIN_TEXTS, "/c")
    assert want.offsets[:16].tolist() == [0, 2, 2, 3, 4, 6, 6, 6, 6, 7, 8, 9, 9, 11, 13, 15] and (want.res.n_arrays, want.res.n_other) == (12, 3)
    c, want, values = both_ways(env, tae.STRUCT_PINS, "/items", "/tags")
    assert want.offsets[:14].tolist() == [0, 0, 0, 2, 2, 2, 2, 4, 4, 4, 5, 5, 5, 5] and [code for code, _ in values].count(0) == 5
    bad = [b'{"c":[[1],[2,3]]}', b'{"c":[[4],tru]}', b'{"c":[[5]]}', b'{"c":[[6]],}', b'{"c":[[7,[8]]]}']
    _, want, _ = both_ways(env, bad, "/c", verdicts=True)
    assert want.offsets[:5].tolist() == [0, 1, 3, 4, 6]
    texts = tae.seeded_documents(5200, 120)
    for j, (list_pointer, sub) in enumerate((("/c", None), ("/items", "/tags"), ("/items", ""), ("/items", "/x/tags"))):
        c, want, _ = both_ways(env, texts, list_pointer, sub, where=(list_pointer, sub), sep=(b"\n", b" ", b"\r\n", b"")[j])
        assert c.w.n > 3 * BLOCK and want.res.n_rows > 100


def tokens_per_row(got):
    return tae.tokens_per_row(got)


def test_block_borders(env):
    """A row whose '[' is a block's last token and whose first element is the next block's first token -- its predecessor
    comes from the halo -- and every position around it; a row's own start on those positions with the offsets it needs."""
    doc = b'{"c":[[7,"s",[8]],[9]]}'   # the rows at f + 4 and f + 14; the first row's elements at f + 5, f + 7, f + 9
    for f in range(BLOCK - 8, BLOCK + 1):
        head, k = tvd.filler(f, f % 2 == 0)
        tail, _ = tvd.filler(30, f % 2 == 1)
        c = Case(env, head + b"\n" + doc + b" " + tail + b"\n", "/c", chain=f % 2 == 1)
        assert int(c.w.first[k]) == f and c.rows["token"].tolist() == [f + 4, f + 14]
        want = c.check(where=f)
        assert tokens_per_row(want) == [[f + 5, f + 7, f + 9], [f + 15]]
    # (f = 1019: the row's '[' is token 1023 and its first element token 1024)


def test_one_array_over_three_blocks(env):
    """One inner array of 2 100 elements -- 4 201 tokens, its middle blocks inside ONE row -- with short rows on either side,
    and nested arrays inside it whose contents are not counted."""
    big = b"[" + b",".join(b"[%d,%d]" % (j, j) if j % 50 == 0 else b"%d" % j for j in range(2100)) + b"]"
    for lead in (1, 300):
        texts = [b'{"c":[[1,2]]}'] * lead + [b'{"c":[[3],' + big + b",[4,5]]}", b'{"c":[[],[6]]}']
        for chain in (False, True):
            c = Case(env, tdk.join(texts, b"\n"), "/c", chain=chain)
            want = c.check(where=(lead, chain))
            t = c.rows["token"].tolist()
            assert (t[lead + 2] - 1) // BLOCK - t[lead + 1] // BLOCK >= 3
            assert int(want.offsets[lead + 2]) - int(want.offsets[lead + 1]) == 2100 and want.res.n_elements == 2 * lead + 1 + 2100 + 2 + 0 + 1


def test_blocks_that_belong_to_no_row(env):
    """Blocks in front of the first row and blocks wholly between two rows, full of [1,2] that belong to no row, take the
    early exits; the rows behind them are exact."""
    noise = b"[" + b",".join([b"[1,2]"] * 520) + b"]"    # 3 121 tokens: whole blocks of candidates without a row
    texts = [b'{"other":' + noise + b"}", b'{"c":[[1]],"pad":' + noise + b',"d":[[5]]}', b'{"c":[[2],[3,3]]}', b'{"pad":' + noise + b"}",
             b'{"c":[[4]]}']
    for chain in (False, True):
        c = Case(env, tdk.join(texts, b"\n"), "/c", chain=chain)
        t = c.rows["token"].tolist()
        assert len(t) == 4 and t[0] // BLOCK >= 3 and t[1] // BLOCK - t[0] // BLOCK >= 3 and t[3] // BLOCK - t[2] // BLOCK >= 3
        want = c.check(where=chain)
        assert want.offsets[:5].tolist() == [0, 1, 2, 4, 5] and want.elements[:5]["bits"].tolist() == [1, 2, 3, 3, 4]


def test_most_rows_in_one_block(env):
    """A row every second token, so about 512 rows own a token of one block: the numbers and [k] arrays of one long array
    through the real chain and uploaded.  Then every token a row, uploaded: 1 024 rows start in one block and the one in
    front of it reaches into it; rows past the window have no dense state."""
    text = b"[" + b",".join(b"[%d]" % j if j % 3 == 0 else b"1" for j in range(1400)) + b"]\n"
    for chain in (False, True):
        c = Case(env, text, "", chain=chain)
        assert c.rows.size == 1400 and c.w.n > 3 * BLOCK
        want = c.check(where=chain)
        assert (want.res.n_arrays, want.res.n_other, want.res.n_elements) == (467, 933, 467)
    text = tae.every_token_a_row()
    w = tdm.WindowArrays(env.oracle, env.nm, text, is_final=True)
    n = w.n
    for lo, hi, step in ((0, n, 1), (0, n, 2), (BLOCK - 1, 2 * BLOCK + 1, 1), (0, n + 5, 1)):
        rows = np.concatenate([tae.record(v) for v in range(lo, hi, step)])
        want = Case(env, text, "", w=w).use(rows).check(where=(lo, hi, step))
        assert want.res.n_arrays == int((w.typ[lo:min(hi, n):step] == ord("[")).sum())


def test_coded_runs_across_blocks_of_rows(env):
    """items[*].tags with runs of structs that have no tags -- records with code 20, and 17 for items that are no objects --
    at the very front, across a block of 256 rows and at the very end: their offsets are the next live row's, or n_elements."""
    item = lambda j: b'{"tags":["t%d","u"]}' % j
    none = lambda j: b'{"sku":%d}' % j if j % 2 else b"%d" % j
    items = [none(j) for j in range(300)] + [item(j) for j in range(150)] + [none(j) for j in range(200)] + [item(j) for j in range(10)] + \
            [none(j) for j in range(300)]
    texts = [b'{"items":[' + b",".join(items[:500]) + b"]}", b'{"items":[' + b",".join(items[500:]) + b"]}"]
    for chain in (False, True):
        c = Case(env, tdk.join(texts, b"\n"), "/items", "/tags", chain=chain)
        assert c.rows.size == 960 and c.rows["code"][:300].tolist() == [17, 20] * 150
        want = c.check(where=chain)
        off = want.offsets[:961].tolist()
        assert off[:301] == [0] * 301 and off[450:651] == [300] * 201 and off[660:] == [320] * 301 and want.res.n_elements == 320
        assert (want.res.n_arrays, want.res.n_other) == (160, 0)


def test_more_rows_than_one_sweep_and_a_second_scan_chunk(env):
    """262 500 rows of [j] and [] -- the kernels over rows take their second trip and rows_ranks its second chunk of block
    sums -- in a window of more than 1 048 577 tokens, which gives items_scan its second chunk."""
    per_line, lines = 100, 2625
    line = lambda k: b'{"c":[' + b",".join(b"[%d]" % ((k + j) % 7) if (k + j) % 25 else b"[]" for j in range(per_line)) + b"]}"
    data = b"\n".join(line(k) for k in range(lines)) + b"\n"
    c = Case(env, data, "/c", chain=True)
    R = per_line * lines
    assert c.rows.size == R == 262500 > SWEEP and c.w.n >= SCAN_CHUNK + 1
    want = c.check(where="sweep", forms=(False,))
    full = (np.arange(R) // per_line + np.arange(R) % per_line) % 25 != 0
    assert (want.res.code, want.res.n_rows, want.res.n_arrays, want.res.n_elements) == (0, R, R, int(full.sum()))
    assert np.array_equal(want.offsets[:R + 1], np.concatenate([[0], np.cumsum(full)]).astype(np.uint64))


def test_one_array_of_70000_elements(env):
    """One row of 70 000 elements between two short ones: 68 blocks of tokens inside one row."""
    big = b"[" + b",".join(b"%d" % j for j in range(70000)) + b"]"
    c = Case(env, b'{"c":[[1],' + big + b',[2,3]]}\n', "/c", chain=True)
    want = c.check(where="70000", forms=(False,))
    assert want.offsets[:4].tolist() == [0, 1, 70001, 70003] and want.elements[1:70001]["bits"].tolist() == list(range(70000))


def test_capacities_and_head_codes(env):
    """elements_capacity exact, one short (MSJ_CAPACITY, the offsets complete, the canary intact) and the layout-only form;
    R > capacity; R == 0; n == 0; d_rows_select with a code, one from a really clipped parent list among them."""
    texts = [b'{"c":[[%d,"s",[1],{"k":2}],[],7]}' % k for k in range(300)]
    data = tdk.join(texts, b"\n")
    for chain in (False, True):
        c = Case(env, data, "/c", chain=chain)
        R, total = 900, 1200
        for kw in (dict(elements_capacity=total), dict(elements_capacity=total - 1), dict(elements_capacity=total // 2), dict(elements_capacity=0),
                   dict(capacity=R + 300, elements_capacity=total + 100)):
            want = c.check(where=(chain, kw), forms=(False,), **kw)
            assert want.res.n_elements == total and want.res.code == (MSJ_CAPACITY if kw["elements_capacity"] < total else 0)
            assert want.untouched(R, min(kw["elements_capacity"], total))
        assert (want.res.n_arrays, want.res.n_other) == (600, 300)
        layout = c.check(where=chain, forms=(True,))
        assert layout.res.code == 0 and layout.res.n_elements == total
        for cap in (R - 1, 0, 1):
            over = c.check(where=(chain, cap), capacity=cap, elements_capacity=total)
            assert over.summary() == (MSJ_CAPACITY, 0, R, 0, 0, 0, 0, MSJ_CAPACITY, 0, 0, 1, 0, 0, 0) and over.untouched(-1, 0)
    # (the chain) one record too few for the parent list: its result has MSJ_CAPACITY, and so has ours
    _, _, _, c.d_rows, c.d_rows_sel = c.list_call(R - 1)
    c.rsel = tse.rows_result(R, MSJ_CAPACITY)
    clipped = c.check(capacity=R, elements_capacity=total)
    assert clipped.summary() == (MSJ_CAPACITY,) + (0,) * 6 + (MSJ_CAPACITY, 0, 0, 1, 0, 0, 0) and clipped.untouched(-1, 0)
    c = Case(env, data, "/c")
    rows = c.rows.copy()
    for code in (9, -1):
        got = c.use(rows, tse.rows_result(R, code)).check(capacity=R, elements_capacity=total)
        assert got.summary() == (code,) + (0,) * 6 + (code, 0, 0, 1, 0, 0, 0) and got.untouched(-1, 0)
    for chain in (False, True):   # R == 0: no list in the window; n == 0: no token
        none = Case(env, b'{"c":7}\n{"other":[[1]]}\n', "/c", chain=chain).check(capacity=3, elements_capacity=2)
        assert none.summary() == (0,) * 10 + (1, 0, 0, 0) and none.offsets[0] == 0 and none.untouched(0, 0)
        c0 = Case(env, b"  \n ", "/c", chain=chain, is_final=False)
        assert c0.w.n == 0 and c0.check(capacity=2, elements_capacity=2).summary() == (0,) * 10 + (1, 0, 0, 0)
    lost = c0.use(rows[:4]).check(capacity=5, elements_capacity=2)   # records of another window over no token at all
    assert lost.summary() == (0, 0, 4, 0, 0, 4, 0, 0, 0, 0, 1, 0, 0, 0) and lost.offsets[:5].tolist() == [0] * 5 and lost.untouched(4, 0)


def test_order_violations_and_hostile_records(env):
    """Uploaded: a descending or equal pair of live rows, also with coded rows between them and across a block of rows --
    MSJ_ERR_BAD_ARGUMENT and nothing written, d_valid and d_offsets included --; then records that lie, partners out of range
    and a row inside a row: nothing faults, and the device follows the twin."""
    w = tae.hostile_window(env.oracle, env.nm)
    c = Case(env, w.data, "", w=w)
    rec, coded = tae.record, tae.coded
    good = [rec(tae.FIRST), rec(tae.SECOND), rec(tae.OTHER), rec(tae.LAST)]
    for order in ([1, 0, 2, 3], [0, 1, 3, 2], [0, 1, 2, 2], [3, 0, 1, 2]):
        for gap in ([], [coded(20)], [coded(17)] * 300):
            rows = []
            for j in order:
                rows += [good[j]] + gap
            got = c.use(np.concatenate(gap + rows)).check(where=(order, len(gap)), elements_capacity=8)
            assert got.res.code == BAD_ARGUMENT and got.res.n_rows == len(gap) * 5 + 4 and got.untouched(-1, 0)
    rows = []
    for g in good:
        rows += [coded(17)] * 300 + [g]
    fine = c.use(np.concatenate(rows + [coded(20)] * 300)).check(where="gaps")
    assert [t for t in tokens_per_row(fine) if t is not None] == [[2, 4], [8, 10], [20], [21]] and fine.offsets[1204:1505].tolist() == [6] * 301
    lying = np.concatenate([rec(tae.OUTER, typ="{"), rec(tae.FIRST), rec(2), rec(tae.SECOND, typ='"'), rec(tae.INNER), coded(17), rec(tae.OTHER + 2),
                            rec(w.n), rec(w.n + 7), rec(tae.NO_TOKEN)])
    want = c.use(lying).check(where="lying")
    assert tokens_per_row(want) == [None, [2], None, None, [11, 13]] + [None] * 5
    nested = c.use(np.concatenate([rec(tae.OUTER), coded(20), rec(tae.SECOND)])).check(where="nested")
    assert tokens_per_row(nested) == [[tae.FIRST, tae.SECOND], None, [8, tae.INNER]]
    for m in (w.n, w.n + 5, tdk.NO_PARTNER, tae.SECOND, tae.SECOND - 1, 0):
        w.match = w.match.copy()
        w.match[tae.SECOND] = m
        edited = Case(env, w.data, "", w=w).use(np.concatenate([rec(tae.FIRST), rec(tae.SECOND), rec(tae.OTHER)])).check(where=m)
        assert tokens_per_row(edited) == [[2, 4], None, [20]]


def test_numbers(env):
    """Number elements with their records, with d_numbers NULL, with d_numbers_result NULL and with a numbers_capacity that
    ends inside the window: the bits, or MSJ_FIELD_NO_BITS and the count of the records written."""
    texts = [b'{"c":[[%d,%d.5],[-1e%d,"x",[%d]]]}' % (k, k, k % 30, k) for k in range(400)]   # 5 elements per line, 3 of them numbers; 4 number tokens
    for chain in (False, True):
        c = Case(env, tdk.join(texts, b"\n"), "/c", chain=chain)
        full = c.check(where=chain)
        assert full.res.n_elements == 2000 and full.res.n_no_bits == 0 and full.elements[5]["bits"] == 1
        for kw, nobits in ((dict(numbers=False), 1200), (dict(numbers_result=False), 1200), (dict(numbers_capacity=800), 600),
                           (dict(numbers_capacity=0), 1200)):
            part = c.check(where=(chain, kw), forms=(False,), **kw)
            assert part.res.n_no_bits == nobits, (kw, part.res.n_no_bits)
        clip = c.check(where=chain, forms=(False,), numbers=False, elements_capacity=700)
        assert clip.res.n_no_bits == 420 and clip.res.code == MSJ_CAPACITY


def test_composition_on_the_device(env):
    """The new elements as the rows of the next call, where they lie on the device: msj_string_column_device over them,
    msj_select_elements_device over them, and this call over them, two more levels down."""
    import torch
    from mojo_simdjson_amd import _lib

    dev = env.dev
    names = ["ab", "c\nd", "", "é\U0001F600", 'q"\\/', "plain" * 9]
    docs = [{"c": [[names[(k + j) % 6] if (k + j) % 4 else k, {"sku": k, "tags": [[names[j % 6]], [k]]}] for j in range(k % 4)]} for k in range(200)]
    texts = [json.dumps(d, ensure_ascii=bool(k % 2)).encode() for k, d in enumerate(docs)]
    data = tdk.join(texts, b"\n")
    for chain in (False, True):
        c = Case(env, data, "/c", chain=chain)
        a = c.a
        want = c.check(where=chain)
        items = [item for d in docs for row in d["c"] for item in row]
        n = len(items)
        assert want.res.n_elements == n > 500
        # the strings among the new elements
        col = tcm.twin_column(env.ctwin, data, want.elements[:n], n)
        offsets, valid, out = tcm.filled(n, col.bytes_capacity)
        res, d_off, d_valid, d_bytes = dev.string_column(a.d_buf, len(data), c.d_elements.unsqueeze(0), 0, c.d_esel,
                                                         d_offsets=torch.from_numpy(offsets.view(np.int64)).to(dev.device),
                                                         d_valid=torch.from_numpy(valid).to(dev.device), d_bytes=torch.from_numpy(out).to(dev.device),
                                                         capacity=n, bytes_capacity=col.bytes_capacity)
        assert (res.code, res.n_rows, res.n_strings, res.total_bytes) == (0, n, col.res.n_strings, col.res.total_bytes)
        assert np.array_equal(d_off.cpu().numpy().view(np.uint64), col.offsets) and np.array_equal(d_bytes.cpu().numpy(), col.data)
        assert col.rows() == [v.encode("utf-8") if isinstance(v, str) else None for v in items]
        # fields by path inside the new elements, and the lists at /tags inside them: this call over a select-elements column
        sel_want = tse.twin_elements(env.twins, c.w, ["/sku", "/tags"], want.elements[:n], want.esel)
        d_sel, d_fields = dev.select_elements(env.paths(["/sku", "/tags"]), a.d_buf, a.length, a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end,
                                              a.d_flags, c.d_elements, c.d_esel, d_numbers=a.d_numbers, numbers_capacity=a.ncap,
                                              d_numbers_result=a.d_num, capacity=n, sync=False)
        got_fields = np.ascontiguousarray(d_fields.cpu().numpy()).view(tsm.FIELD_DTYPE).reshape(2, -1)
        assert np.array_equal(got_fields[:, :n], np.stack([sel_want.column(0)[:n], sel_want.column(1)[:n]]))
        tags = c.use(sel_want.column(1)[:n].copy(), sel_want.res)
        tags.d_rows, tags.d_rows_sel = d_fields[1], d_sel
        level2 = tags.check(where=(chain, "tags"))
        assert level2.res.n_arrays == n // 2 and level2.res.n_elements == n
        # ... and once more over its own output: the [name] and [k] lists
        rows3, sel3 = tae.next_level(level2)
        deep = c.use(rows3, sel3)
        deep.d_rows, deep.d_rows_sel = tags.d_elements, tags.d_esel
        level3 = deep.check(where=(chain, "deep"))
        assert level3.res.n_arrays == n and level3.res.n_elements == n
        host = np.frombuffer(c.w.data, dtype=np.uint8)
        leaves = [tsm.field_value(r, host, c.w.idx, c.w.end) for r in level3.elements[:n]]
        assert leaves == [v for d in docs for row in d["c"] for item in row if isinstance(item, dict) for lst in item["tags"] for v in lst]
    assert _lib.MsjSelectDocumentsResult.from_buffer_copy(deep.d_esel.cpu().numpy().tobytes()).n_documents == n


def test_bad_arguments_and_check_order(env):
    """Each is refused with nothing launched: the outputs keep what was in them.  Two faults at once: missing arrays are
    judged before the size, the size before outputs and alignment."""
    import torch

    dev = env.dev
    c = Case(env, b'{"c":[[1,"b"],[2]]}\n', "/c", chain=True)
    a = c.a
    sent = torch.full((6,), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    esel = torch.full((6,), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    off = torch.full((8,), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    val = torch.full((16,), 0x5A, dtype=torch.uint8, device=dev.device)
    out = torch.full((8, 2), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    tensors = dict(idx=a.d_idx, type=a.d_type, depth=a.d_depth, match=a.d_match, end=a.d_end, flags=a.d_flags, numbers=a.d_numbers, num=a.d_num,
                   rows=c.d_rows, sel=c.d_rows_sel, off=off, val=val, out=out, res=sent, esel=esel)

    def call(**kw):
        p = {k: t.data_ptr() for k, t in tensors.items()}
        p.update(ctx=dev.ctx, n=a.n, ncap=a.ncap, cap=2, room=8)
        p.update(kw)
        return dev.lib.msj_array_elements_device(p["ctx"], p["idx"], p["n"], p["type"], p["depth"], p["match"], p["end"], p["flags"], p["numbers"],
                                                 p["ncap"], p["num"], p["rows"], p["sel"], p["off"], p["val"], p["cap"], p["out"], p["room"],
                                                 p["res"], p["esel"], dev._stream())

    assert call(n=1 << 31) == MSJ_CAPACITY
    for name in ("ctx", "res", "sel", "idx", "type", "depth", "match", "end", "flags", "rows", "off", "val", "out", "numbers"):
        assert call(**{name: None}) == BAD_ARGUMENT, name
    assert call(esel=tensors["sel"].data_ptr()) == BAD_ARGUMENT and call(out=tensors["rows"].data_ptr()) == BAD_ARGUMENT
    for name, step in (("idx", 8), ("depth", 4), ("match", 8), ("end", 4), ("numbers", 8), ("rows", 8), ("out", 8), ("type", 4), ("flags", 1),
                       ("num", 4), ("sel", 4), ("off", 4), ("res", 4), ("esel", 4)):
        assert call(**{name: tensors[name].data_ptr() + step}) == BAD_ARGUMENT, name
    # two faults, as tests/test_check_order.py states them for the siblings
    assert call(type=None, n=1 << 31) == BAD_ARGUMENT
    assert call(n=1 << 31, idx=tensors["idx"].data_ptr() + 4) == MSJ_CAPACITY
    assert call(out=None, depth=tensors["depth"].data_ptr() + 4) == BAD_ARGUMENT
    torch.cuda.synchronize()
    for t in (sent, esel, off, out):
        assert bool((t == tvd.SENTINEL).all())
    assert bool((val == 0x5A).all()) and dev.lib.msj_array_elements_workspace_bytes(0, 0) > 0
    # an unaligned d_valid, no d_elements_select, no number records, the layout-only form, and no capacity at all with NULL arrays
    assert call(val=val.data_ptr() + 1, esel=None, numbers=None, ncap=0, num=None) == 0
    torch.cuda.synchronize()
    t0 = int(c.rows["token"][0])
    assert sent.cpu().numpy().tolist() == [0, 2, 2, 3, 0, 2] and val.cpu().numpy()[1:3].tolist() == [1, 1] and off.cpu().numpy()[:3].tolist() == [0, 2, 3]
    assert out.cpu().numpy()[:3, 1].tolist() == [t0 + 1 | ord("l") << 32 | 64 << 40, t0 + 3 | ord('"') << 32, t0 + 7 | ord("l") << 32 | 64 << 40]
    assert bool((esel == tvd.SENTINEL).all()) and bool((out[3:] == tvd.SENTINEL).all())
    assert call(out=None, room=0) == 0 and call(rows=None, off=None, val=None, cap=0, out=None, room=0) == 0
    torch.cuda.synchronize()
    assert sent.cpu().numpy().tolist() == [MSJ_CAPACITY, 2, 0, 0, 0, 0] and esel.cpu().numpy().tolist() == [MSJ_CAPACITY, 0, 1, 0, 0, 0]


def test_document_stream_lists_of_lists(env):
    """A few hundred lines of NDJSON through windows of 4 096 bytes, DocumentStream(select=["/coordinates", "/items"]):
    Window.elements("/coordinates").elements().numbers() and Window.elements("/items").select(["/tags"]).elements("/tags")
    .strings() / .to_python() equal json.loads on every line; the element buffers have to grow in every other window."""
    import torch
    from mojo_simdjson_amd.document_stream import DocumentStream, ListColumn

    dev = env.dev
    coords = lambda k: [[k + j, j + 0.5] for j in range(k % 5)] + ([7, [], [[k]]] if k % 6 == 0 else [])
    items = lambda k: [{"sku": "s%d" % j, "tags": ["t%d\n" % (k + j), "é"][:(k + j) % 3]} if (k + j) % 4 else [{"sku": 1}, 7, {"tags": 5}][(k + j) % 3]
                       for j in range(k % 4)]
    lines = [json.dumps({"id": k, "coordinates": coords(k) if k % 9 else "none", "items": items(k), "pad": "p" * (k % 40)},
                        ensure_ascii=bool(k % 2)).encode() for k in range(300)]
    lines[100] = b'{"id":100,"coordinates":[[1,2],tru],"items":[]}'
    data = b"\n".join(lines) + b"\n"
    docs = [None if k == 100 else json.loads(line) for k, line in enumerate(lines)]
    rows_c = [item for d in docs if d and isinstance(d["coordinates"], list) for item in d["coordinates"]]
    rows_t = [item.get("tags") if isinstance(item, dict) else None for d in docs if d for item in d["items"]]
    stream = DocumentStream(dev, tvd.upload(dev, data), len(data), window=4096, select=["/coordinates", "/items"])
    got_c, got_f, got_t, got_s, windows = [], [], [], [], 0
    for win in stream:
        outer = win.elements("/coordinates")
        inner = outer.elements(elements_capacity=1 if windows % 2 else None)   # (1: the buffer has to grow)
        assert isinstance(inner, ListColumn) and inner.parent is outer and outer.parent is None and inner.window is win
        assert inner.offsets.shape == (outer.n_elements + 1,) and inner.valid.shape == (outer.n_elements,) and inner.fields.shape == (inner.n_elements, 2)
        assert inner.offsets.dtype == torch.int64 and inner.valid.dtype == torch.bool and inner.fields.is_cuda
        got_c += inner.to_python()
        values, valid = inner.numbers(torch.float64)
        off = inner.offsets.cpu().tolist()
        flat = [v if ok else None for v, ok in zip(values.cpu().tolist(), valid.cpu().tolist())]
        got_f += [flat[off[r]:off[r + 1]] for r in range(outer.n_elements)]
        fields = win.elements("/items").select(["/tags"])
        tags = fields.elements("/tags", elements_capacity=None if windows % 2 else 1)
        assert tags.parent is fields and tags.offsets.shape == (fields.n_elements + 1,) and tags.elements().n_elements == 0
        got_t += tags.to_python()
        s_off, s_bytes, s_valid = tags.strings()
        so, raw, ok, off = s_off.cpu().tolist(), s_bytes.cpu().numpy().tobytes(), s_valid.cpu().tolist(), tags.offsets.cpu().tolist()
        strings = [raw[so[j]:so[j + 1]].decode("utf-8") if ok[j] else None for j in range(tags.n_elements)]
        got_s += [strings[off[r]:off[r + 1]] for r in range(fields.n_elements)]
        windows += 1
    assert windows >= 6 and len(got_c) == len(rows_c) > 400 and len(got_t) == len(rows_t) > 300
    for r, (g, w) in enumerate(zip(got_c, rows_c)):
        assert (g == w and isinstance(w, list)) or (g is None and not isinstance(w, list)), (r, g, w)
    is_num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
    assert got_f == [[float(v) if is_num(v) else None for v in w] if isinstance(w, list) else [] for w in rows_c]
    for r, (g, w) in enumerate(zip(got_t, rows_t)):
        assert (g == w and isinstance(w, list)) or (g is None and not isinstance(w, list)), (r, g, w)
    assert got_s == [w if isinstance(w, list) else [] for w in rows_t] and sum(len(s) for s in got_s) > 200
