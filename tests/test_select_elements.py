"""Fields by path inside the elements of a list column on the device (msj_select_elements_device,
csrc/select_elements_kernel.hip).

Expected values come from the host twin of the same arithmetic (tests/select_elements_math_host.cpp), which
tests/test_select_elements_math.py holds against the definition written in Python.  Device output is compared with the twin
over the WHOLE d_fields array and the 48-byte result (both start from the same fill, with 64 bytes of canary behind
n_paths * capacity records, so a store the twin does not make shows).  Arrays and records come both ways: from the oracles
and the twins, uploaded, and from the real chain (shard, stage2_prep, documents, number_values, validate_documents,
select_documents, array_column), whose device results the call reads.  A block of se_level is 1 024 tokens; the kernels over
rows sweep 1 024 blocks of 256 rows.
"""
import json

import numpy as np
import pytest

from tests import helpers
from tests import select_reference as ref
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

BLOCK = 1024             # tokens per workgroup of se_level (csrc/tape_block.h: kBlock)
SWEEP = 1024 * 256       # rows one sweep of se_init / se_step / se_finish covers
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


def device_elements(a, paths, d_rows, d_rows_sel, capacity, numbers=True, numbers_result=True, numbers_capacity=None):
    """msj_select_elements_device over the arrays `a`, d_fields filled like the twin's with its canary, d_result with a fill
    of its own -> (tsm.Selected, d_fields, d_result)"""
    import torch
    from mojo_simdjson_amd import _lib

    dev = a.dev
    d_fields = torch.from_numpy(tsm.filled_fields(paths.n_paths, capacity).view(np.int64).reshape(-1, 2)).to(dev.device)
    d_res = torch.full((48,), 0x5A, dtype=torch.uint8, device=dev.device)
    ncap = (a.ncap if numbers_capacity is None else numbers_capacity) if numbers else 0
    dev.select_elements(paths, a.d_buf, a.length, a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end, a.d_flags, d_rows, d_rows_sel,
                        d_numbers=a.d_numbers if numbers else None, numbers_capacity=ncap, d_numbers_result=a.d_num if numbers_result else None,
                        d_fields=d_fields, capacity=capacity, d_result=d_res, sync=False)
    res = _lib.MsjSelectDocumentsResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
    fields = np.ascontiguousarray(d_fields.cpu().numpy()).view(tsm.FIELD_DTYPE).reshape(-1)
    return tsm.Selected(res, fields, paths.n_paths, capacity), d_fields, d_res


class Case:
    """One window both ways: the oracles' arrays and the twins' element records of the list at `list_pointer`; on the device
    either all of that uploaded, or the real chain with the real select and array-column calls."""

    def __init__(self, env, data, list_pointer, chain, verdicts=False, is_final=True, w=None):
        self.env, self.chain = env, chain
        self.w = w = tdm.WindowArrays(env.oracle, env.nm, data, is_final=is_final) if w is None else w
        self.verdict_rows = tdm.twin_documents(env.twins.v, w, 100)[0] if verdicts else None
        self.lists, self.rows, self.esel = tse.element_rows(env.twins, w, list_pointer, verdicts=self.verdict_rows)
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
        else:
            self.a = tsd.Uploaded(env.dev, w, self.verdict_rows)
            self.d_rows, self.d_rows_sel = upload_rows(env.dev, self.rows, self.esel)

    def use(self, rows, rows_select=None):
        """Other records than the list's own (uploaded)"""
        self.rows = np.ascontiguousarray(rows)
        self.esel = tse.rows_result(self.rows.size) if rows_select is None else rows_select
        self.d_rows, self.d_rows_sel = upload_rows(self.env.dev, self.rows, self.esel)
        return self

    def check(self, pointers, where=None, capacity=None, **kw):
        """The call on the device against the twin -> the twin's Selected"""
        want = tse.twin_elements(self.env.twins, self.w, pointers, self.rows, self.esel, capacity=capacity, **kw)
        got, self.d_fields, self.d_result = device_elements(self.a, self.env.paths(pointers), self.d_rows, self.d_rows_sel, want.capacity, **kw)
        tsd.same(got, want, (where, self.chain, kw))
        return want


def both_ways(env, texts, list_pointer, pointers, verdicts=False, where=None):
    """A window of documents both ways in, against the twin and (through it) the definition -> {(p, r): (code, value)}"""
    data = tdk.join(texts, b"\n")
    codes = None
    for chain in (False, True):
        c = Case(env, data, list_pointer, chain, verdicts=verdicts)
        assert c.w.D == len(texts)
        want = c.check(pointers, where=where)
        codes = [code for code, _ in c.verdict_rows] if verdicts else None
    _, rows = tse.definition(texts, list_pointer, pointers, codes)
    return c, tse.check_against_definition(c.w, want, pointers, rows)


def test_pins_and_corpus(env):
    """Every pin of the CPU test in one window, the root lists, 16 paths at once, documents with a verdict code and a seeded
    corpus: both ways in, against the twin and the definition."""
    c, got = both_ways(env, tse.PINS, "/items", tse.PIN_PATHS)
    assert c.rows.size == 22 and got[(0, 7)] == (0, 2) and got[(0, 8)] == (20, None) and got[(0, 10)] == (0, 1) and got[(2, 18)] == (0, {"w": 3})
    c, got = both_ways(env, tse.ROOT_PINS, "", ["/sku", ""])
    assert [got[(0, r)] for r in range(c.rows.size)] == [(0, 2), (20, None), (0, 1), (17, None), (0, [2])]
    both_ways(env, tse.PINS + tse.seeded_lists(7, 40), "/items", tse.SIXTEEN)
    bad = [b'{"items":[{"sku":1},{"sku":2}]}', b'{"items":[{"sku":3},tru]}', b'{"items":[{"sku":4}]}', b'{"items":[{"sku":5}],}', b'{"items":[{"sku":6}]}']
    c, got = both_ways(env, bad, "/items", ["/sku"], verdicts=True)
    assert [got[(0, r)] for r in range(c.rows.size)] == [(0, 1), (0, 2), (0, 4), (0, 6)]
    c, got = both_ways(env, tse.seeded_lists(4100, 150), "/items", tse.CORPUS_PATHS)
    assert c.rows.size > 300 and c.w.n > 3 * BLOCK


def test_block_borders(env):
    """An element whose opener is the last token of a block and whose keys lie in the next; a key that is a block's last
    token with its ':' in the halo; and every position around them."""
    doc = b'{"items":[{"sku":1,"qty":"x"},{"qty":2}]}'   # the first element at f + 4, its keys at f + 5 and f + 9, the second at f + 14
    for f in range(BLOCK - 11, BLOCK - 2):
        head, k = tvd.filler(f, f % 2 == 0)
        tail, _ = tvd.filler(30, f % 2 == 1)
        c = Case(env, head + b"\n" + doc + b" " + tail + b"\n", "/items", chain=f % 2 == 1)
        assert int(c.w.first[k]) == f and c.rows["token"].tolist() == [f + 4, f + 14]
        want = c.check(["/sku", "/qty", "/nope"], where=f)
        assert want.column(0)[:2]["code"].tolist() == [0, 20] and want.column(1)[:2]["token"].tolist() == [f + 11, f + 17]
    # (f = 1019: the opener is token 1023; f = 1018 and 1014: the keys "sku" and "qty" are)


def test_one_element_over_three_blocks(env):
    """One element of more than 3 x 1 024 tokens: a whole block lies inside a single row.  The wanted key is in its last
    block, a same-named key of a nested object in its first."""
    pad = b"[" + b",".join([b"0"] * 1700) + b"]"
    big = b'{"x":{"sku":"inner","w":{"w":1}},"pad":' + pad + b',"sku":"last","dims":{"w":2}}'
    texts = [b'{"items":[{"sku":"a"}]}', b'{"items":[{"sku":"b"},' + big + b',{"sku":"c"}]}', b'{"items":[{"dims":{"w":3}}]}']
    for chain in (False, True):
        c = Case(env, tdk.join(texts, b"\n"), "/items", chain)
        t = c.rows["token"].tolist()
        assert len(t) == 5 and t[3] - t[2] > 3 * BLOCK and (t[3] - 1) // BLOCK - t[2] // BLOCK >= 3
        want = c.check(["/sku", "/dims/w", "/x/w/w", "/pad"], where=chain)
        data = np.frombuffer(c.w.data, dtype=np.uint8)
        value = lambda p, r: tsm.field_value(want.column(p)[r], data, c.w.idx, c.w.end)
        assert [value(0, r) for r in range(5)] == ["a", "b", "last", "c", None] and [value(1, r) for r in range(5)] == [None, None, 2, None, 3]
        assert value(2, 2) == 1 and want.column(0)[2]["token"] // BLOCK > t[2] // BLOCK + 2 and len(value(3, 2)) == 1700


def test_most_rows_in_one_block(env):
    """[1,1,1,...] mixed with {"k":j} elements: a block overlapped by the most rows the array column can produce (an element
    every second token), through the real chain and uploaded.  Then every token a row, uploaded: 1 024 rows own a token of
    one block, and the row at the block's last token overlaps it too."""
    text, pointers = tse.every_token_a_row()
    for chain in (False, True):
        c = Case(env, text, "", chain)
        assert c.rows.size == 700 and np.diff(c.rows["token"][:60].astype(np.int64)).min() == 2
        want = c.check(pointers, where=chain)
        assert want.res.n_found == 234 + 700 and want.column(0)[:700:3]["bits"].tolist() == list(range(0, 700, 3))
    n = c.w.n
    assert n > 2 * BLOCK + 64
    for lo, hi in ((0, n), (BLOCK - 1, 2 * BLOCK), (0, n + 5)):   # (the last: rows past the window, which have no state word)
        rows = np.concatenate([tse.record(v) for v in range(lo, hi)])
        want = Case(env, text, "", False, w=c.w).use(rows).check(pointers, where=(lo, hi))
        assert want.res.n_found == int((c.w.typ[lo:hi] == ord("{")).sum()) + min(hi, n) - lo


def test_block_between_rows(env):
    """Blocks that no row reaches (in front of the first row) and blocks that lie wholly between two rows' objects -- full of
    keys of the same name that belong to no row -- take the early exit; the blocks behind them have matches."""
    noise = b"[" + b",".join([b'{"sku":0}'] * 520) + b"]"    # 3 121 tokens: whole blocks of keys without a row
    texts = [b'{"other":' + noise + b"}", b'{"items":[{"sku":1}],"pad":' + noise + b',"sku":5}', b'{"items":[{"sku":2},{"sku":3}]}',
             b'{"pad":' + noise + b"}", b'{"items":[{"sku":4}]}']
    for chain in (False, True):
        c = Case(env, tdk.join(texts, b"\n"), "/items", chain)
        t = c.rows["token"].tolist()
        assert len(t) == 4 and t[0] // BLOCK >= 3 and t[1] // BLOCK - t[0] // BLOCK >= 3 and t[3] // BLOCK - t[2] // BLOCK >= 3
        want = c.check(["/sku", "/pad"], where=chain)
        assert want.column(0)[:4]["bits"].tolist() == [1, 2, 3, 4] and want.column(0)[:4]["code"].tolist() == [0] * 4
        assert want.column(1)[:4]["code"].tolist() == [20] * 4


def test_more_rows_than_one_sweep(env):
    """Over 262 144 elements of {"a":j}, about 1.6 M tokens: the kernels over rows wrap, and se_finish's block counts add up."""
    per_line, lines = 100, SWEEP // 100 + 4
    line = lambda k: b'{"items":[' + b",".join(b'{"a":%d}' % ((k + j) % 7) for j in range(per_line)) + b"]}"
    data = b"\n".join(line(k) for k in range(lines)) + b"\n"
    c = Case(env, data, "/items", True)
    R = per_line * lines
    assert c.rows.size == R > SWEEP and c.w.n > 1500000
    want = c.check(["/a", "/b", ""], where="sweep")
    assert (want.res.code, want.res.n_documents, want.res.n_found, want.res.n_no_bits) == (0, R, 2 * R, 0)
    assert np.array_equal(want.column(0)[:R]["bits"], (np.arange(R) // per_line + np.arange(R) % per_line) % 7)
    assert want.column(1)[:R]["code"].tolist() == [20] * R and np.array_equal(want.column(2)[:R]["token"], c.rows["token"])


def test_head_codes(env):
    """R > capacity; d_rows_select with MSJ_CAPACITY from a really clipped array-column call; a descending pair; R = 0; n = 0:
    the result alone, the records and their canary as they were filled."""
    texts = [b'{"items":[{"sku":1},{"sku":2},{"sku":3}]}', b'{"items":[{"sku":4}]}']
    data = tdk.join(texts, b"\n")
    for chain in (False, True):
        c = Case(env, data, "/items", chain)
        for cap in (3, 0, 1):
            over = c.check(["/sku", ""], where=cap, capacity=cap)
            assert over.summary() == (MSJ_CAPACITY, 0, 4, 2, 0, 0, 0) and over.untouched(0)
        assert c.check(["/sku", ""], capacity=4).res.n_found == 8
    # (the chain) one record too few for the elements: the list's result has MSJ_CAPACITY, and so has ours
    _, _, _, c.d_rows, c.d_rows_sel = c.list_call(3)
    c.esel = tse.rows_result(4, MSJ_CAPACITY)
    clipped = c.check(["/sku", ""], capacity=6)
    assert clipped.summary() == (MSJ_CAPACITY, 0, 0, 0, 0, 0, 0) and clipped.untouched(0)
    c = Case(env, data, "/items", False)
    rows = c.rows.copy()
    for a, b in ((0, 1), (2, 3), (0, 3)):
        bad = rows.copy()
        bad[[a, b]] = bad[[b, a]]
        got = c.use(bad).check(["/sku", ""], where=(a, b), capacity=6)
        assert got.summary() == (BAD_ARGUMENT, 0, 4, 2, 0, 0, 0) and got.untouched(0)
    for code in (9, -1):
        got = c.use(rows, tse.rows_result(4, code)).check(["/sku"], capacity=4)
        assert got.summary() == (code, 0, 0, 0, 0, 0, 0) and got.untouched(0)
    for chain in (False, True):   # R = 0: no list in the window; n = 0: no token
        none = Case(env, b'{"items":7}\n{"other":[{"sku":1}]}\n', "/items", chain).check(["/sku", ""], capacity=3)
        assert none.summary() == (0, 0, 0, 2, 0, 0, 0) and none.untouched(0)
        c0 = Case(env, b"  \n ", "/items", chain, is_final=False)
        assert c0.w.n == 0 and c0.check(["/sku", ""], capacity=2).summary() == (0, 0, 0, 2, 0, 0, 0)
    lost = c0.use(rows).check(["/sku", ""], capacity=5)   # records of another window over no token at all
    assert lost.summary() == (0, 0, 4, 2, 0, 0, 0) and lost.column(1)[:4]["code"].tolist() == [17] * 4 and lost.untouched(4)


def test_numbers(env):
    """Number fields with their records, with d_numbers NULL, with d_numbers_result NULL and with a numbers_capacity that ends
    inside the window: the bits, or MSJ_FIELD_NO_BITS, and n_no_bits."""
    texts = [b'{"items":[{"i":%d,"f":%d.5,"s":"x"},{"i":-1e%d}]}' % (k, k, k % 30) for k in range(300)]
    for chain in (False, True):
        c = Case(env, tdk.join(texts, b"\n"), "/items", chain)
        full = c.check(["/i", "/f", "/s"], where=chain)
        assert (full.res.n_found, full.res.n_no_bits) == (600 + 300 + 300, 0) and full.column(0)[:4]["bits"].tolist()[::2] == [0, 1]
        for kw, nobits in ((dict(numbers=False), 900), (dict(numbers_result=False), 900), (dict(numbers_capacity=300), 600), (dict(numbers_capacity=0), 900)):
            part = c.check(["/i", "/f", "/s"], where=(chain, kw), **kw)
            assert (part.res.n_found, part.res.n_no_bits) == (1200, nobits), kw


def test_hostile_records(env):
    """Records no array-column call writes, uploaded: token >= n, '{' records on other tokens, other tags on objects, a code,
    partners out of range, one row inside another.  Nothing faults, and the device follows the twin."""
    w = tse.hostile_window(env.oracle, env.nm)
    c = Case(env, w.data, "/items", False, w=w)
    t = c.rows["token"].tolist()
    rec = tse.record
    lying = np.concatenate([rec(t[0]), rec(t[0] + 1), rec(t[1], typ="["), rec(t[3]), rec(t[4], typ='"'), rec(w.n), rec(w.n + 7),
                            rec(tse.NO_TOKEN, typ="", code=20)])
    want = c.use(lying).check(["/sku", ""])
    assert want.column(0)[:8]["code"].tolist() == [0] + [17] * 6 + [20] and want.column(1)[:8]["code"].tolist() == [0] * 5 + [17, 17, 20]
    outer = int(w.first[1]) + 1
    nested = c.use(np.concatenate([rec(outer), rec(outer + 7)])).check(["/a", "/b", "/in", "/in/a", ""])
    assert nested.column(1)[:2]["code"].tolist() == [20, 0] and nested.column(0)[:2]["bits"].tolist() == [1, 2]
    for m in (w.n, w.n + 5, tdk.NO_PARTNER, t[1], t[1] - 1, 0):
        w.match = w.match.copy()
        w.match[t[1]] = m
        edited = Case(env, w.data, "/items", False, w=w)
        want = edited.check(["/sku", "/sku/x"], where=m)
        assert want.column(0)[:edited.rows.size]["code"].tolist().count(17) >= 1


def test_string_column_over_a_new_column(env):
    """msj_string_column_device over one of the new columns with the new d_result, unchanged: the string-column twin's
    offsets, validity and bytes."""
    import torch

    dev = env.dev
    names = ["ab", "c\nd", "", "é\U0001F600", 'q"\\/', "plain" * 9]
    texts = [json.dumps({"items": [{"name": names[(k + j) % 6]} if (k + j) % 5 else {"name": k, "nick": "n"} for j in range(k % 6)]},
                        ensure_ascii=bool(k % 2)).encode() for k in range(200)]
    data = tdk.join(texts, b"\n")
    for chain in (False, True):
        c = Case(env, data, "/items", chain)
        R = c.rows.size
        want = c.check(["/nick", "/name"], where=chain)
        col = tcm.twin_column(env.ctwin, data, want.column(1)[:R], R)
        offsets, valid, out = tcm.filled(R, col.bytes_capacity)
        d_fields = c.d_fields[:2 * R].reshape(2, R, 2)
        res, d_off, d_valid, d_bytes = dev.string_column(c.a.d_buf, len(data), d_fields, 1, c.d_result,
                                                         d_offsets=torch.from_numpy(offsets.view(np.int64)).to(dev.device),
                                                         d_valid=torch.from_numpy(valid).to(dev.device), d_bytes=torch.from_numpy(out).to(dev.device),
                                                         capacity=R, bytes_capacity=col.bytes_capacity)
        assert (res.code, res.n_rows, res.n_strings, res.total_bytes) == (0, R, col.res.n_strings, col.res.total_bytes)
        assert np.array_equal(d_off.cpu().numpy().view(np.uint64), col.offsets) and np.array_equal(d_valid.cpu().numpy(), col.valid)
        assert np.array_equal(d_bytes.cpu().numpy(), col.data)
        items = [item for text in texts for item in json.loads(text)["items"]]
        assert col.rows() == [v["name"].encode("utf-8") if isinstance(v["name"], str) else None for v in items] and col.res.n_escaped > 30


def test_bad_arguments(env):
    """Each is refused with nothing launched: the outputs keep what was in them."""
    import torch

    dev = env.dev
    c = Case(env, b'{"items":[{"sku":1},{"sku":"b"}]}\n', "/items", True)
    a = c.a
    paths = env.paths(["/sku"])
    sent = torch.full((6,), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    out = torch.full((8, 2), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    tensors = dict(buf=a.d_buf, idx=a.d_idx, type=a.d_type, depth=a.d_depth, match=a.d_match, end=a.d_end, flags=a.d_flags, numbers=a.d_numbers,
                   num=a.d_num, rows=c.d_rows, sel=c.d_rows_sel, out=out, res=sent)

    def call(**kw):
        p = {k: t.data_ptr() for k, t in tensors.items()}
        p.update(ctx=dev.ctx, paths=paths.handle, n=a.n, len=a.length, ncap=a.ncap, cap=2)
        p.update(kw)
        return dev.lib.msj_select_elements_device(p["ctx"], p["paths"], p["buf"], p["len"], p["idx"], p["n"], p["type"], p["depth"], p["match"],
                                                  p["end"], p["flags"], p["numbers"], p["ncap"], p["num"], p["rows"], p["sel"], p["out"], p["cap"],
                                                  p["res"], dev._stream())

    assert call(n=1 << 31) == MSJ_CAPACITY and call(len=(1 << 32) + 1) == MSJ_CAPACITY
    for name in ("paths", "res", "sel", "buf", "idx", "type", "depth", "match", "end", "flags", "rows", "out", "numbers"):
        assert call(**{name: None}) == BAD_ARGUMENT, name
    assert call(res=tensors["sel"].data_ptr()) == BAD_ARGUMENT
    for name, step in (("idx", 8), ("depth", 4), ("match", 8), ("end", 4), ("numbers", 8), ("rows", 8), ("out", 8), ("type", 4), ("flags", 1),
                       ("num", 4), ("sel", 4), ("res", 4)):
        assert call(**{name: tensors[name].data_ptr() + step}) == BAD_ARGUMENT, name
    torch.cuda.synchronize()
    assert bool((sent == tvd.SENTINEL).all()) and bool((out == tvd.SENTINEL).all()) and dev.lib.msj_select_elements_workspace_bytes(0, 0, 1) > 0
    # no number records, and no capacity at all with NULL records
    assert call(numbers=None, ncap=0, num=None) == 0
    torch.cuda.synchronize()
    assert sent.cpu().numpy().tolist() == [0, 2, 1, 2, 1, 0]
    assert out.cpu().numpy()[:2, 1].tolist() == [int(c.rows["token"][0]) + 3 | ord("l") << 32 | 64 << 40, int(c.rows["token"][1]) + 3 | ord('"') << 32]
    assert bool((out[2:] == tvd.SENTINEL).all())
    assert call(rows=None, out=None, cap=0) == 0
    torch.cuda.synchronize()
    assert sent.cpu().numpy().tolist() == [MSJ_CAPACITY, 2, 1, 0, 0, 0]


def test_document_stream_list_of_structs(env):
    """A few hundred lines of NDJSON through windows of 4 096 bytes, DocumentStream(select=["/items", "/id"]):
    Window.elements("/items").select([...]).to_python() equals json.loads on every line; .numbers(), .strings(), .values() and
    .column() agree with it."""
    import torch
    from mojo_simdjson_amd.document_stream import DocumentStream, ElementFields

    dev = env.dev
    rng_items = lambda k: [{"sku": "s%d\n" % (k + j), "qty": k * j, "dims": {"w": j + 0.5}} if (k + j) % 4 else
                           [{"qty": 1.5, "dims": 3}, 7, {"sku": None, "sku ": "x"}, {}][(k + j) % 3] for j in range(k % 6)]
    lines = [json.dumps({"id": k, "items": rng_items(k) if k % 9 else "none", "pad": "p" * (k % 40)}, ensure_ascii=bool(k % 2)).encode() for k in range(300)]
    lines[100] = b'{"id":100,"items":[{"sku":"bad"},tru]}'
    data = b"\n".join(lines) + b"\n"
    pointers = ["/sku", "/qty", "/dims/w"]
    want = []
    for k, line in enumerate(lines):
        items = None if k == 100 else json.loads(line)["items"]
        if not isinstance(items, list):
            want.append(None)
            continue
        rows = [[ref.lookup(ref.decode(json.dumps(item).encode()), p) for p in pointers] for item in items]
        want.append([{p: v for p, (code, v) in zip(pointers, row) if code == 0} for row in rows])
    stream = DocumentStream(dev, tvd.upload(dev, data), len(data), window=4096, select=["/items", "/id"])
    got, qty, names, windows = [], [], [], 0
    for win in stream:
        col = win.elements("/items")
        ef = col.select(pointers)
        assert isinstance(ef, ElementFields) and ef.fields.shape == (3, col.n_elements, 2) and ef.fields.dtype == torch.int64 and ef.fields.is_cuda
        assert ef.d_select.shape == (48,) and ef.column("/qty").shape == (col.n_elements,)
        got += ef.to_python()
        values, valid = ef.numbers("/qty", torch.int64)
        qty += [v if ok else None for v, ok in zip(values.cpu().tolist(), valid.cpu().tolist())]
        s_off, s_bytes, s_valid = ef.strings(0)
        so, raw, ok = s_off.cpu().tolist(), s_bytes.cpu().numpy().tobytes(), s_valid.cpu().tolist()
        strings = [raw[so[j]:so[j + 1]].decode("utf-8") if ok[j] else None for j in range(col.n_elements)]
        assert strings == [v if isinstance(v, str) else None for v in ef.values("/sku")]
        names += strings
        again = col.select(ef.paths)     # compiled paths are taken as they are
        assert again.fields.equal(ef.fields)
        windows += 1
    assert windows >= 6 and len(got) == len(lines)
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), k
        assert w is None or (len(g) == len(w) and all(tsm.same_value(x, y) for x, y in zip(g, w))), (k, g, w)
    flat = [item for w in want if w for item in w]
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)
    assert qty == [item["/qty"] if is_int(item.get("/qty")) else None for item in flat]
    assert names == [item["/sku"] if isinstance(item.get("/sku"), str) else None for item in flat] and sum(n is not None for n in names) > 200
