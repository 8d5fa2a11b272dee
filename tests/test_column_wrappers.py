"""The five column methods of Stage1Device (mojo_simdjson_amd/device.py) as wrappers: string_column, raw_column, array_column,
array_elements and object_entries share how they default d_offsets / d_valid / d_result, how they size the output from a
layout-only first call, and what they return.  This file pins that, not the kernels: one window of four NDJSON lines, far
below one block of 1 024 tokens, with a string field, a list, a list of lists, an object whose keys are data, and one path that
no document has.

For every method and for both a path that has values and the missing one, these ways of calling give the same offsets,
validity, payload (bytes, elements, keys and values, cut at the total the call reports) and the same result struct:
    1. everything defaulted -- the layout-only first call plus the real call
    2. the caller's d_offsets / d_valid / output buffers, no capacity named
    3. capacities named, no buffers
    4. sync=False: the device tensor that holds the result, its bytes those of the synchronous result
and the layout-only form alone returns None for the payload and the same counts.  The payload of the first way is held
against the definitions the per-call test modules already have in Python (tests/select_reference.py and the `definition`
functions of the *_math test modules), which know nothing of this code.
"""
import numpy as np
import pytest

from mojo_simdjson_amd.document_stream import FIELD_DTYPE, field_value
from tests import select_reference as ref
from tests import test_array_column_math as tac
from tests import test_array_elements_math as tae
from tests import test_object_entries_math as tom
from tests import test_raw_column_math as trm
from tests import test_select_documents as tsd
from tests import test_select_math as tsm
from tests import test_string_column_math as tcm
from tests import test_tape_documents_math as tdk

pytestmark = pytest.mark.gpu

LINES = [b'{"s":"red","l":[1,"a"],"ll":[[1,2],[]],"m":{"color":"red","size":"L"}}',
         b'{"s":"a\\nb","l":[],"ll":[[3]],"m":{}}',
         b'{"s":7,"l":[true,null,2.5],"ll":[],"m":{"k":{"x":1},"k2":[1]}}',
         b'{"l":[{"a":1}],"ll":[[4,[5]],7],"m":"no"}']
POINTERS = ["/s", "/l", "/ll", "/m", "/zz"]
MISSING = POINTERS.index("/zz")
ROOM = 3   # records per path beyond the documents: the default capacity is the rows of d_fields, not the rows the call finds


@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    d = Stage1Device(0)
    yield d
    d.close()


class Win:
    """The window through the real chain and the select call, and host copies of what the definitions read"""

    def __init__(self, dev):
        self.dev, self.data = dev, tdk.join(LINES, b"\n")
        self.a = a = tsd.FromChain(dev, self.data, False, False)
        assert a.n < 1024
        self.D = len(LINES)
        self.numbers = dict(d_numbers=a.d_numbers, numbers_capacity=a.ncap, d_numbers_result=a.d_num)
        self.tokens = (a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end, a.d_flags)
        self.d_sel, self.d_fields = dev.select_documents(dev.compile_paths(POINTERS), a.d_buf, a.length, *self.tokens, a.d_first, a.d_docs,
                                                         capacity=self.D + ROOM, sync=False, **self.numbers)
        self.host = (np.frombuffer(self.data, dtype=np.uint8), a.d_idx.cpu().numpy().view(np.uint32)[:a.n], a.d_end.cpu().numpy().view(np.uint32)[:a.n])

    def value(self, rec):
        return field_value(rec, *self.host)


@pytest.fixture(scope="module")
def win(dev):
    return Win(dev)


def records(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(FIELD_DTYPE).reshape(-1)


class Method:
    """One column method: call(**kw) with everything but the outputs bound; outs: the keywords of its payload tensors; room:
    the keyword of their capacity; switch: the keyword that turns the payload off; total: the result field that sizes it;
    rows: the capacity the defaults take"""

    def __init__(self, call, outs, room, switch, total, rows):
        self.call, self.outs, self.room, self.switch, self.total, self.rows = call, outs, room, switch, total, rows

    def new(self, dev, n):
        import torch

        if self.outs == ("d_bytes",):
            return torch.full((n,), 0x77, dtype=torch.uint8, device=dev.device)
        return torch.full((n, 2), 0x77, dtype=torch.int64, device=dev.device)


def held(dev, m):
    """The ways of calling `m` against each other -> (result, offsets[R + 1], valid[R], [payload[total] per output])"""
    import torch

    k = len(m.outs)
    first = m.call()
    res = first[0]
    R, total = int(res.n_rows), int(getattr(res, m.total))

    def view(got):
        assert len(got) == len(first)
        payload = [t.cpu().numpy()[:total] for t in got[3:3 + k]]
        selects = [t.cpu().numpy().tobytes() for t in got[3 + k:]]
        return got[1].cpu().numpy()[:R + 1], got[2].cpu().numpy()[:R], payload, selects

    def same(got, where):
        a, b = view(got), view(first)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (where, a[:2], b[:2])
        assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2])) and a[3] == b[3], where

    # 1: sized from the layout-only first call, never an empty tensor
    assert all(t.shape[0] == max(total, 1) for t in first[3:3 + k]) and first[1].numel() == m.rows + 1 and first[2].numel() == max(m.rows, 1)
    # the layout-only form alone
    layout = m.call(**{m.switch: False})
    assert all(t is None for t in layout[3:3 + k]) and bytes(layout[0]) == bytes(res)
    assert np.array_equal(layout[1].cpu().numpy()[:R + 1], first[1].cpu().numpy()[:R + 1])
    assert np.array_equal(layout[2].cpu().numpy()[:R], first[2].cpu().numpy()[:R])
    # 2: the caller's buffers, no capacity named
    mine = {name: m.new(dev, max(total, 1)) for name in m.outs}
    d_off, d_valid = torch.empty(m.rows + 1, dtype=torch.int64, device=dev.device), torch.empty(max(m.rows, 1), dtype=torch.uint8, device=dev.device)
    second = m.call(d_offsets=d_off, d_valid=d_valid, **mine)
    assert second[1] is d_off and second[2] is d_valid and all(second[3 + j] is mine[name] for j, name in enumerate(m.outs))
    assert bytes(second[0]) == bytes(res)
    same(second, 2)
    # 3: capacities named, no buffers
    third = m.call(capacity=m.rows, **{m.room: total})
    assert bytes(third[0]) == bytes(res) and all(t.shape[0] == max(total, 1) for t in third[3:3 + k])
    same(third, 3)
    # 4: nothing waited for
    fourth = m.call(sync=False)
    assert isinstance(fourth[0], torch.Tensor) and fourth[0].is_cuda and fourth[0].cpu().numpy().tobytes() == bytes(res)
    same(fourth, 4)
    assert res.code == 0
    off, valid, payload, _ = view(first)
    return res, off.tolist(), valid.tolist(), payload


def empty(dev, m, rows):
    """The missing path: a total of 0, the buffer still made with one element, every row empty and not valid"""
    res, off, valid, payload = held(dev, m)
    assert (int(res.n_rows), int(getattr(res, m.total))) == (rows, 0) and off == [0] * (rows + 1) and valid == [0] * rows
    assert all(p.shape[0] == 0 for p in payload)


def string_column(w, p):
    return Method(lambda **kw: w.dev.string_column(w.a.d_buf, w.a.length, w.d_fields, p, w.d_sel, **kw),
                  ("d_bytes",), "bytes_capacity", "strings", "total_bytes", w.D + ROOM)


def raw_column(w, p):
    return Method(lambda **kw: w.dev.raw_column(w.a.d_buf, w.a.length, w.a.d_idx, w.a.n, w.a.d_type, w.a.d_match, w.a.d_end, w.a.d_flags,
                                                w.d_fields[p], w.d_sel, **kw),
                  ("d_bytes",), "bytes_capacity", "text", "total_bytes", w.D + ROOM)


def array_column(w, p):
    return Method(lambda **kw: w.dev.array_column(*w.tokens, w.a.d_first, w.a.d_docs, w.d_fields, p, w.d_sel, **w.numbers, **kw),
                  ("d_elements",), "elements_capacity", "elements", "n_elements", w.D + ROOM)


def array_elements(w, d_rows, d_rows_sel):
    return Method(lambda **kw: w.dev.array_elements(*w.tokens, d_rows, d_rows_sel, **w.numbers, **kw),
                  ("d_elements",), "elements_capacity", "elements", "n_elements", d_rows.shape[0])


def object_entries(w, d_rows, d_rows_sel):
    return Method(lambda **kw: w.dev.object_entries(*w.tokens, d_rows, d_rows_sel, **w.numbers, **kw),
                  ("d_keys", "d_values"), "entries_capacity", "entries", "n_entries", d_rows.shape[0])


def path_values(pointer):
    return [ref.lookup(ref.decode(text), pointer) for text in LINES]


def test_string_column(dev, win):
    res, off, valid, (data,) = held(dev, string_column(win, 0))
    want_off, want_valid, want, n_strings, n_other = tcm.definition(path_values("/s"))
    assert (off, valid, data.tobytes()) == (want_off, want_valid, want) and want == b"reda\nb"
    assert (res.n_strings, res.n_escaped, res.n_other) == (n_strings, 1, n_other)
    empty(dev, string_column(win, MISSING), win.D)


def test_raw_column(dev, win):
    p = POINTERS.index("/m")
    res, off, valid, (data,) = held(dev, raw_column(win, p))
    recs = records(win.d_fields[p])[:win.D]
    want = [trm.expect_verbatim(win.data, win.host[1], r) if r["code"] == 0 else None for r in recs]
    assert want == [b'{"color":"red","size":"L"}', b"{}", b'{"k":{"x":1},"k2":[1]}', b'"no"']
    assert [data.tobytes()[off[k]:off[k + 1]] if valid[k] else None for k in range(win.D)] == want
    assert (res.n_values, res.n_containers, res.total_bytes) == (4, 3, sum(len(t) for t in want))
    empty(dev, raw_column(win, MISSING), win.D)


def check_lists(win, res, off, valid, elements, values):
    want_off, want_valid, items, n_other = tac.definition(values)
    assert (off, valid) == (want_off, want_valid) and len(items) == res.n_elements > 0
    got = [win.value(r) for r in elements.view(FIELD_DTYPE).reshape(-1)]
    assert all(tsm.same_value(g, x) for g, x in zip(got, items)), (got, items)
    assert (res.n_arrays, res.n_other, res.n_no_bits) == (sum(want_valid), n_other, 0)


def test_array_column(dev, win):
    res, off, valid, (elements,) = held(dev, array_column(win, POINTERS.index("/l")))
    check_lists(win, res, off, valid, elements, path_values("/l"))
    empty(dev, array_column(win, MISSING), win.D)


def test_array_elements(dev, win):
    _, _, _, d_rows, d_rows_sel = win.dev.array_column(*win.tokens, win.a.d_first, win.a.d_docs, win.d_fields, POINTERS.index("/ll"), win.d_sel,
                                                       sync=False, **win.numbers)
    values = tae.definition(LINES, "/ll")
    assert d_rows.shape[0] == len(values) == 5
    res, off, valid, (elements,) = held(dev, array_elements(win, d_rows, d_rows_sel))
    check_lists(win, res, off, valid, elements, values)
    empty(dev, array_elements(win, win.d_fields[MISSING], win.d_sel), win.D)


def test_object_entries(dev, win):
    res, off, valid, (keys, values) = held(dev, object_entries(win, win.d_fields[POINTERS.index("/m")], win.d_sel))
    want_off, want_valid, pairs, n_other = tom.definition(tom.definition_rows(LINES, ("doc", "/m")))
    assert (off, valid) == (want_off, want_valid) and len(pairs) == res.n_entries == 4
    keys, values = keys.view(FIELD_DTYPE).reshape(-1), values.view(FIELD_DTYPE).reshape(-1)
    for j, (key, want) in enumerate(pairs):
        assert win.value(keys[j]) == key and tsm.same_value(win.value(values[j]), tom.plain(want)), (j, key, want)
    assert (res.n_objects, res.n_other, res.n_no_bits) == (sum(want_valid), n_other, 0)
    empty(dev, object_entries(win, win.d_fields[MISSING], win.d_sel), win.D)
