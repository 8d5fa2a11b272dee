"""A selected path's arrays as a list column on the device (msj_array_column_device, csrc/array_column_kernel.hip).

Expected values come from the host twin of the same arithmetic (tests/array_column_math_host.cpp), which
tests/test_array_column_math.py holds against the definition written in Python.  Device output is compared with the twin
over the WHOLE d_offsets, d_valid and d_elements arrays (both start from the same fill, with 64 bytes of canary behind each
capacity, so a store the twin does not make shows).  Arrays and records come both ways: from the oracles and the select
twin, uploaded, and from the real chain (shard, stage2_prep, documents, number_values, validate_documents,
select_documents), whose device results the call reads.  A block of ac_count / ac_emit is 1 024 tokens; ac_scan takes
1 024 blocks per round.
"""
import json

import numpy as np
import pytest

from tests import helpers
from tests import select_reference as ref
from tests import test_array_column_math as tac
from tests import test_number_math as tnm
from tests import test_select_documents as tsd
from tests import test_select_math as tsm
from tests import test_string_column_math as tcm
from tests import test_tape_documents as ttd
from tests import test_tape_documents_math as tdk
from tests import test_validate_documents as tvd
from tests import test_validate_documents_math as tdm
from tests import test_validate_math as tvm

pytestmark = pytest.mark.gpu

BLOCK = 1024               # tokens per workgroup of ac_count / ac_emit (csrc/tape_block.h: kBlock)
SCAN_CHUNK = 1024 * BLOCK  # tokens whose block counts ac_scan takes in one round
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
        self.vtwin, self.stwin, self.atwin, self.ctwin = tdm.load_twin(), tsm.load_twin(), tac.load_twin(), tcm.load_twin()
        self._paths = {}

    def paths(self, pointers):
        key = tuple(pointers)
        if key not in self._paths:
            self._paths[key] = self.dev.compile_paths(pointers)
        return self._paths[key]


def device_lists(a, d_fields, p, d_sel, want, numbers=True, numbers_result=True, numbers_capacity=None):
    """msj_array_column_device over the arrays `a` with the twin's capacities, its arrays filled like the twin's with their
    canaries -> (tac.Lists, d_elements, d_elements_select)"""
    import torch
    from mojo_simdjson_amd import _lib

    dev = a.dev
    offsets, valid, elements = tac.filled(want.capacity, want.elements_capacity, want.elements is None)
    d_off = torch.from_numpy(offsets.view(np.int64)).to(dev.device)
    d_valid = torch.from_numpy(valid).to(dev.device)
    d_el = torch.from_numpy(elements.view(np.int64).reshape(-1, 2)).to(dev.device) if elements is not None else None
    d_esel = torch.full((48,), 0x5A, dtype=torch.uint8, device=dev.device)
    ncap = (a.ncap if numbers_capacity is None else numbers_capacity) if numbers else 0
    d_res, _, _, _, _ = dev.array_column(a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end, a.d_flags, a.d_first, a.d_docs, d_fields, p, d_sel,
                                         d_numbers=a.d_numbers if numbers else None, numbers_capacity=ncap,
                                         d_numbers_result=a.d_num if numbers_result else None, d_offsets=d_off, d_valid=d_valid, d_elements=d_el,
                                         capacity=want.capacity, elements_capacity=want.elements_capacity, elements=elements is not None,
                                         d_elements_select=d_esel, sync=False)
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


def upload_records(dev, records, D, code=0):
    """Columns of records as d_fields of shape (n_paths, rows, 2), and a select result for D documents"""
    records = [np.concatenate([np.ascontiguousarray(r), np.zeros(1, dtype=tsm.FIELD_DTYPE)]) for r in records]   # (never an empty tensor)
    d_fields = ttd.to_device(dev, np.concatenate(records)).reshape(len(records), -1, 2)
    d_sel = ttd.to_device(dev, np.frombuffer(bytes(tac.select_result(D, code, len(records))), dtype=np.uint8))
    return d_fields, d_sel


class Case:
    """One window both ways: the oracles' arrays, the verdict twin's rows and the select twin's records; on the device
    either all of that uploaded, or the real chain and the real select call."""

    def __init__(self, env, data, pointers, chain, verdicts=False, is_final=False, max_depth=100):
        self.env, self.pointers = env, pointers
        self.w = w = tdm.WindowArrays(env.oracle, env.nm, data, is_final=is_final)
        self.rows = tdm.twin_documents(env.vtwin, w, max_depth)[0] if verdicts else None
        self.selected = tsm.twin_select(env.stwin, w, pointers, verdicts=self.rows)
        self.records = [self.selected.column(p)[:w.D].copy() for p in range(len(pointers))]
        if chain:
            self.a = a = tsd.FromChain(env.dev, data, is_final, verdicts, max_depth)
            assert a.n == w.n
            self.d_sel, self.d_fields = env.dev.select_documents(
                env.paths(pointers), a.d_buf, a.length, a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end, a.d_flags, a.d_first, a.d_docs,
                d_numbers=a.d_numbers, numbers_capacity=a.ncap, d_numbers_result=a.d_num, d_verdicts=a.d_verdicts, capacity=w.D + 3, sync=False)
        else:
            self.a = tsd.Uploaded(env.dev, w, self.rows)
            self.d_fields, self.d_sel = upload_records(env.dev, self.records, w.D)

    def values(self, docs):
        """(code, value) per (p, document) from the reference, the select twin's records held against it"""
        return tsm.check_against_reference(self.w, self.selected, self.pointers, docs, codes=[c for c, _ in self.rows] if self.rows else None)

    def check(self, p=0, where=None, forms=(True, False), **kw):
        """Path p's column on the device against the twin, in the layout-only form and with the elements -> the twin's Lists"""
        for layout_only in forms:
            want = tac.twin_lists(self.env.atwin, self.w, self.records[p], layout_only=layout_only, **kw)
            dkw = {k: v for k, v in kw.items() if k in ("numbers", "numbers_result", "numbers_capacity")}
            got, _, _ = device_lists(self.a, self.d_fields, p, self.d_sel, want, **dkw)
            same(got, want, (where, p, layout_only, kw))
        return want


def rows_of(lists):
    """The element tokens per row of a complete twin column, None for a row that is no array"""
    D = int(lists.res.n_rows)
    off = lists.offsets[:D + 1].tolist()
    return [lists.elements[off[k]:off[k + 1]]["token"].tolist() if lists.valid[k] else None for k in range(D)]


def test_pins_and_corpus(env):
    """The pins of the CPU test and six streams of its corpus: both ways in, every pointer, against the twin and the
    definition."""
    pins = (tdk.join(tac.PINS, b"\n"), tac.PINS, ["", "/a", "/a/b", "/zz"])
    for j, (data, docs, pointers) in enumerate([pins] + tsm.corpus()[:6]):
        for chain in (False, True):
            c = Case(env, data, pointers, chain, verdicts=bool(j % 2))
            assert c.w.D == len(docs)
            values = c.values(docs) if chain else None
            for p in range(len(pointers)):
                want = c.check(p, where=(j, chain))
                if chain:
                    tac.check_against_definition(c.w, want, [values[(p, k)] for k in range(c.w.D)])
    # [[],[]] has two elements: the ']' of a nested [] is none
    want = Case(env, b"[[],[]]\n[[]]\n", [""], True).check()
    assert want.offsets[:3].tolist() == [0, 2, 3] and want.elements[:3]["type"].tolist() == [ord("[")] * 3


def test_block_borders(env):
    """An element on every token position from 3 in front of a block border to 3 behind it -- the '[' or ',' in front of it
    sits in the block before -- and a document's first token on every one of those positions."""
    doc = b'{"a":[7,"s",[8]]}'   # elements at f + 4, f + 6, f + 8
    for lead in (4, 6, 0):
        for at in range(BLOCK - 3, BLOCK + 4):
            head, k = tvd.filler(at - lead, at % 2 == 0)
            tail, _ = tvd.filler(30, at % 2 == 1)
            c = Case(env, head + b"\n" + doc + b" " + tail + b"\n", ["/a", ""], chain=at % 2 == 0)
            assert int(c.w.first[k]) == at - lead and c.w.typ[at - lead] == ord("{")
            want = c.check(0, where=(lead, at))
            f = at - lead
            assert rows_of(want)[k] == [f + 4, f + 6, f + 8] and want.res.n_arrays == 1
            root = c.check(1, where=(lead, at))   # the filler's [1,2,3] are rows here, the object is none
            assert rows_of(root)[k] is None and root.res.n_other > 0 and root.res.n_elements == 3 * root.res.n_arrays


def test_array_over_three_blocks(env):
    """One array of 2 100 elements -- 4 201 tokens, three block borders inside it -- with short documents on either side."""
    big = b"[" + b",".join(b"%d" % j for j in range(2100)) + b"]"
    for lead in (1, 700):
        docs = [b"[1,2]"] * lead + [big] + [b"[3]", b"[]", b"[4,5]"]
        for chain in (False, True):
            c = Case(env, b"\n".join(docs) + b"\n", [""], chain)
            want = c.check(where=(lead, chain))
            assert want.res.n_elements == 2 * lead + 2100 + 3 and int(want.offsets[lead + 1]) - int(want.offsets[lead]) == 2100
            f = int(c.w.first[lead])
            assert (f + 4200) // BLOCK - f // BLOCK >= 3
            assert rows_of(want)[lead] == list(range(f + 1, f + 4200, 2))
            assert want.elements[2 * lead:2 * lead + 2100]["bits"].tolist() == list(range(2100))


def test_blocks_without_an_element(env):
    """1 200 consecutive rows that are empty arrays, non-arrays and missing keys -- whole blocks hold no element and still
    write their 0 and their documents' offsets -- between rows that have elements."""
    kinds = [b'{"a":[]}', b'{"a":1}', b'{"b":[1]}', b'{"a":{"a":[2]}}']
    docs = [b'{"a":[1,2]}'] * 3 + [kinds[k % 4] for k in range(1200)] + [b'{"a":["x"]}'] * 2
    for chain in (False, True):
        c = Case(env, b"\n".join(docs) + b"\n", ["/a"], chain)
        want = c.check(where=chain)
        assert want.offsets[3:1204].tolist() == [6] * 1201 and want.offsets[1205] == 8 and want.res.n_arrays == 5 + 300
        tokens = set(t // BLOCK for row in rows_of(want) if row for t in row)
        empty = [b for b in range(c.w.T // BLOCK) if b not in tokens]
        starts = set((c.w.first[:c.w.D] // BLOCK).tolist())
        assert len(empty) >= 4 and all(b in starts for b in empty)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_row_counts(env, n):
    """1, 255, 256, 257 and 513 rows of 0 to 4 elements: both ways in."""
    docs = [b'{"a":[' + b",".join(b'"%d"' % j for j in range(k % 5)) + b"]}" for k in range(n)]
    for chain in (False, True):
        want = Case(env, b"\n".join(docs) + b"\n", ["/a"], chain).check(where=(n, chain))
        assert want.res.n_arrays == n and want.res.n_elements == sum(k % 5 for k in range(n))


def test_invalid_document_across_a_border(env):
    """A document with a verdict code whose array straddles a block border, with d_verdicts: no row, no element; its
    neighbours are exact.  Without d_verdicts the select call looks it up and its elements are there."""
    bad = b'{"a":[1,2,3,4,5,6,tru]}'
    for at in (BLOCK - 8, BLOCK - 2):
        head, k = tvd.filler(at, True)
        data = head + b"\n" + bad + b'\n{"a":[9]}\n'
        for chain in (False, True):
            c = Case(env, data, ["/a"], chain, verdicts=True)
            assert c.rows[k][0] == tvm.T_ATOM and int(c.w.first[k]) == at
            want = c.check(where=(at, chain))
            assert rows_of(want)[k:k + 2] == [None, [int(c.w.first[k + 1]) + 4]] and want.res.n_elements == 1
        free = Case(env, data, ["/a"], True, verdicts=False).check(where=at)
        assert len(rows_of(free)[k]) == 7 and free.res.n_elements == 8


def test_capacities(env):
    """capacity one short and 0: nothing but the results.  elements_capacity one short, half and 0: offsets and validity
    complete, the elements clipped.  More room than needed.  A select result with a code, and one of another window."""
    docs = [b'{"a":[%d,"s",[1],{"k":2}]}' % k for k in range(300)] + [b'{"a":7}', b'{"a":[]}']
    for chain in (False, True):
        c = Case(env, b"\n".join(docs) + b"\n", ["/a"], chain)
        D, total = c.w.D, 1200
        for kw in (dict(elements_capacity=total - 1), dict(elements_capacity=total // 2), dict(elements_capacity=0), dict(capacity=D - 1),
                   dict(capacity=0, elements_capacity=5), dict(capacity=D + 300, elements_capacity=total + 100)):
            want = c.check(where=chain, forms=(False,), **kw)
            if "capacity" not in kw:
                assert want.res.code == MSJ_CAPACITY and want.res.n_elements == total and want.untouched(D, kw["elements_capacity"])
        assert want.res.code == 0 and want.res.n_other == 1
        over = c.check(where=chain, capacity=D - 1)
        assert over.summary()[:7] == (MSJ_CAPACITY, 0, D, 0, 0, 0, 0) and over.untouched(-1, 0)
    # (uploaded) a select result with a code, and one that counts another number of documents
    for kw, code in ((dict(sel_code=MSJ_CAPACITY), MSJ_CAPACITY), (dict(sel_code=9), 9), (dict(sel_D=D - 1), BAD_ARGUMENT), (dict(sel_D=D + 1), BAD_ARGUMENT)):
        c.d_fields, c.d_sel = upload_records(env.dev, c.records, kw.get("sel_D", D), kw.get("sel_code", 0))
        want = c.check(where=kw, capacity=D + 2, elements_capacity=total, **kw)
        assert want.summary() == (code, 0, 0, 0, 0, 0, 0, code, 0, 0, 1, 0, 0, 0) and want.untouched(-1, 0)
    # the real select call with one record too few: its result has MSJ_CAPACITY, and so has the column's
    a = c.a = tsd.FromChain(env.dev, b"\n".join(docs) + b"\n", False, False)
    c.d_sel, c.d_fields = env.dev.select_documents(env.paths(["/a"]), a.d_buf, a.length, a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end,
                                                   a.d_flags, a.d_first, a.d_docs, d_numbers=a.d_numbers, numbers_capacity=a.ncap,
                                                   d_numbers_result=a.d_num, capacity=D - 1, sync=False)
    want = c.check(sel_code=MSJ_CAPACITY, capacity=D, elements_capacity=total)
    assert want.res.code == MSJ_CAPACITY and want.untouched(-1, 0)
    # no document at all: offsets[0] and a zero result
    for data in (b'{"a":[1,"abc', b"  \n "):
        none = Case(env, data, ["/a"], True).check(capacity=3, elements_capacity=2)
        assert none.summary() == (0,) * 10 + (1, 0, 0, 0) and none.offsets[0] == 0 and none.untouched(0, 0)


def test_numbers(env):
    """Number elements with their records, with d_numbers NULL, with d_numbers_result NULL and with a numbers_capacity that
    ends inside the window (the first 200 documents' records): the bits, or MSJ_FIELD_NO_BITS and the count of the records
    written."""
    docs = [b'{"v":[%d,%d.5,-1e%d,"x",[%d]]}' % (k, k, k % 30, k) for k in range(400)]   # 5 elements each, 3 of them numbers; 4 number tokens
    for chain in (False, True):
        c = Case(env, b"\n".join(docs) + b"\n", ["/v"], chain)
        full = c.check(where=chain)
        assert full.res.n_elements == 2000 and full.res.n_no_bits == 0
        assert full.elements[:3]["type"].tolist() == [ord("l"), ord("d"), ord("d")] and full.elements[5]["bits"] == 1
        for kw, nobits in ((dict(numbers=False), 1200), (dict(numbers_result=False), 1200), (dict(numbers_capacity=800), 600),
                           (dict(numbers_capacity=0), 1200)):
            part = c.check(where=(chain, kw), forms=(False,), **kw)
            assert part.res.n_no_bits == nobits, (kw, part.res.n_no_bits)
        clip = c.check(where=chain, forms=(False,), numbers=False, elements_capacity=700)
        assert clip.res.n_no_bits == 420 and clip.res.code == MSJ_CAPACITY


def test_scan_takes_a_second_chunk(env):
    """100 000 lines of {"a":[1,2,3]}: 1 100 000 tokens, more than the 1 048 576 whose block counts ac_scan takes in its
    first round."""
    D = 100000
    data = b'{"a":[1,2,3]}\n' * D
    c = Case(env, data, ["/a"], True)
    assert c.w.n == 11 * D and c.w.n > SCAN_CHUNK + 4 * BLOCK
    want = c.check()
    assert want.offsets[:D + 1].tolist() == list(range(0, 3 * D + 1, 3)) and want.res.n_elements == 3 * D
    assert want.elements[:3 * D]["token"].tolist() == [11 * k + j for k in range(D) for j in (4, 6, 8)]
    assert want.elements[:3 * D]["bits"].tolist() == [1, 2, 3] * D


def test_hostile_records(env):
    """Records no select call writes, uploaded: token >= n, a token of another document, a '[' record on a '{' token, the
    wrong tag, a code.  None is an array, the good rows beside them are exact."""
    c = Case(env, tdk.join(tac.HOSTILE, b"\n"), [""], False)
    records, good = tac.hostile_records(c.w)
    c.records = [records]
    c.d_fields, c.d_sel = upload_records(env.dev, c.records, c.w.D)
    want = c.check()
    assert [k for k in range(c.w.D) if want.valid[k]] == good and want.res.n_other == 5


def test_string_elements(env):
    """String elements, plain and escaped, through msj_string_column_device over d_elements with d_elements_select: the
    strings of the definition.  A clipped list hands on MSJ_CAPACITY, and the string call refuses it."""
    import torch
    from mojo_simdjson_amd import _lib

    dev = env.dev
    texts = ["ab", "c\nd", "", "é\U0001F600", "q\"\\/", "plain" * 9]
    docs = [json.dumps({"t": [texts[(k + j) % 6] if (k + j) % 7 else k for j in range(k % 5)]}, ensure_ascii=bool(k % 2)).encode() for k in range(300)]
    data = b"\n".join(docs) + b"\n"
    for chain in (False, True):
        c = Case(env, data, ["/t"], chain)
        d_buf = c.a.d_buf
        want = tac.twin_lists(env.atwin, c.w, c.records[0])
        got, d_el, d_esel = device_lists(c.a, c.d_fields, 0, c.d_sel, want)
        same(got, want, chain)
        items = [v for doc in docs for v in json.loads(doc)["t"]]
        n = len(items)
        assert want.res.n_elements == n > 500
        col = tcm.twin_column(env.ctwin, data, want.elements[:n], n)
        offsets, valid, out = tcm.filled(n, col.bytes_capacity)
        res, d_off, d_valid, d_bytes = dev.string_column(d_buf, len(data), d_el.unsqueeze(0), 0, d_esel,
                                                         d_offsets=torch.from_numpy(offsets.view(np.int64)).to(dev.device),
                                                         d_valid=torch.from_numpy(valid).to(dev.device), d_bytes=torch.from_numpy(out).to(dev.device),
                                                         capacity=n, bytes_capacity=col.bytes_capacity)
        assert (res.code, res.n_rows, res.n_strings, res.total_bytes) == (0, n, col.res.n_strings, col.res.total_bytes)
        assert np.array_equal(d_off.cpu().numpy().view(np.uint64), col.offsets) and np.array_equal(d_valid.cpu().numpy(), col.valid)
        assert np.array_equal(d_bytes.cpu().numpy(), col.data)
        assert col.rows() == [v.encode("utf-8") if isinstance(v, str) else None for v in items] and col.res.n_escaped > 50
        # one record short: the list is clipped, its select result says so, the string call writes a zero result with that code
        clip = tac.twin_lists(env.atwin, c.w, c.records[0], elements_capacity=n - 1)
        got, d_el, d_esel = device_lists(c.a, c.d_fields, 0, c.d_sel, clip)
        same(got, clip, chain)
        assert clip.esel.code == MSJ_CAPACITY
        res, d_off, d_valid, d_bytes = dev.string_column(d_buf, len(data), d_el.unsqueeze(0), 0, d_esel,
                                                         d_offsets=torch.from_numpy(offsets.view(np.int64)).to(dev.device),
                                                         d_valid=torch.from_numpy(valid).to(dev.device), d_bytes=torch.from_numpy(out).to(dev.device),
                                                         capacity=n, bytes_capacity=col.bytes_capacity)
        assert (res.code, res.n_rows, res.n_strings, res.total_bytes) == (MSJ_CAPACITY, 0, 0, 0)
        assert np.array_equal(d_off.cpu().numpy().view(np.uint64), offsets) and np.array_equal(d_bytes.cpu().numpy(), out)
    assert _lib.MsjSelectDocumentsResult.from_buffer_copy(d_esel.cpu().numpy().tobytes()).n_documents == n


def test_bad_arguments(env):
    """Each is refused with nothing launched: the outputs keep what was in them."""
    import torch

    dev = env.dev
    c = Case(env, b'{"a":[1,"b"]}\n{"a":[2]}\n', ["/a"], True)
    a = c.a
    sent = torch.full((6,), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    esel = torch.full((6,), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    off = torch.full((8,), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    val = torch.full((16,), 0x5A, dtype=torch.uint8, device=dev.device)
    out = torch.full((8, 2), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    tensors = dict(idx=a.d_idx, type=a.d_type, depth=a.d_depth, match=a.d_match, end=a.d_end, flags=a.d_flags, first=a.d_first, docs=a.d_docs,
                   numbers=a.d_numbers, num=a.d_num, col=c.d_fields, sel=c.d_sel, off=off, val=val, out=out, res=sent, esel=esel)

    def call(**kw):
        p = {k: t.data_ptr() for k, t in tensors.items()}
        p.update(n=a.n, ncap=a.ncap, cap=2, room=8)
        p.update(kw)
        return dev.lib.msj_array_column_device(dev.ctx, p["idx"], p["n"], p["type"], p["depth"], p["match"], p["end"], p["flags"], p["first"],
                                               p["docs"], p["numbers"], p["ncap"], p["num"], p["col"], p["sel"], p["off"], p["val"], p["cap"],
                                               p["out"], p["room"], p["res"], p["esel"], dev._stream())

    assert call(n=1 << 31) == MSJ_CAPACITY
    for name in ("res", "sel", "docs", "idx", "type", "depth", "match", "end", "flags", "first", "col", "off", "val", "out", "numbers"):
        assert call(**{name: None}) == BAD_ARGUMENT, name
    for name, step in (("idx", 8), ("depth", 4), ("match", 8), ("end", 4), ("numbers", 8), ("col", 8), ("out", 8), ("type", 4), ("flags", 1),
                       ("docs", 4), ("num", 4), ("sel", 4), ("off", 4), ("res", 4), ("esel", 4), ("first", 2)):
        assert call(**{name: tensors[name].data_ptr() + step}) == BAD_ARGUMENT, name
    torch.cuda.synchronize()
    for t in (sent, esel, off, out):
        assert bool((t == tvd.SENTINEL).all())
    assert bool((val == 0x5A).all()) and dev.lib.msj_array_column_workspace_bytes(0, 0) > 0
    # an unaligned d_valid, no d_elements_select, no number records, the layout-only form, and no capacity at all with NULL arrays
    assert call(val=val.data_ptr() + 1, esel=None, numbers=None, ncap=0, num=None) == 0
    torch.cuda.synchronize()
    assert sent.cpu().numpy().tolist() == [0, 2, 2, 3, 0, 2] and val.cpu().numpy()[1:3].tolist() == [1, 1] and off.cpu().numpy()[:3].tolist() == [0, 2, 3]
    assert out.cpu().numpy()[:3, 1].tolist() == [4 | ord("l") << 32 | 64 << 40, 6 | ord('"') << 32, 13 | ord("l") << 32 | 64 << 40]
    assert bool((esel == tvd.SENTINEL).all()) and bool((out[3:] == tvd.SENTINEL).all())
    assert call(out=None, room=0) == 0 and call(col=None, off=None, val=None, cap=0, out=None, room=0) == 0
    torch.cuda.synchronize()
    assert sent.cpu().numpy().tolist() == [MSJ_CAPACITY, 2, 0, 0, 0, 0] and esel.cpu().numpy().tolist() == [MSJ_CAPACITY, 0, 1, 0, 0, 0]


def test_document_stream_elements(env):
    """A few hundred lines of NDJSON through windows of 4 096 bytes, DocumentStream(select=["/tags", "/id"]):
    Window.elements("/tags").to_python(), .numbers() for both dtypes and .strings() equal the reference's value of every
    document; the element buffer has to grow in every other window.  Without select the call raises."""
    import torch
    from mojo_simdjson_amd.document_stream import DocumentStream

    dev = env.dev
    kinds = [lambda k: [k, k + 1], lambda k: ["t%d" % k, "e\né", ""], lambda k: [], lambda k: [k + 0.5, "x", None, True, [k], {"a": [k]}],
             lambda k: k, lambda k: {"tags": [1]}, lambda k: list(range(k % 40))]
    lines = [json.dumps({"id": k, "tags": kinds[k % 7](k), "pad": "p" * (k % 50)}, ensure_ascii=bool(k % 2)).encode() for k in range(400)]
    lines[11] = b'{"id":11}'
    lines[200] = b'{"id":200,"tags":[1,2,tru]}'
    lines[301] = b'{"tags":["first"],"tags":[2]}'
    data = b"\n".join(lines) + b"\n"
    decoded = [None if k == 200 else ref.decode(x) for k, x in enumerate(lines)]
    want = [(tvm.T_ATOM, None) if d is None else ref.lookup(d, "/tags") for d in decoded]
    want = [v if c == 0 and isinstance(v, list) else None for c, v in want]
    stream = DocumentStream(dev, tvd.upload(dev, data), len(data), window=4096, select=["/tags", "/id"])
    rows, ints, floats, strings, windows = [], [], [], [], 0
    for win in stream:
        col = win.elements("/tags", elements_capacity=1 if windows % 2 else None)   # (1: the buffer has to grow)
        assert col.offsets.dtype == torch.int64 and col.fields.dtype == torch.int64 and col.valid.dtype == torch.bool and col.fields.is_cuda
        assert col.offsets.shape == (win.n_documents + 1,) and col.valid.shape == (win.n_documents,) and col.fields.shape == (col.n_elements, 2)
        off = col.offsets.cpu().tolist()
        assert off[0] == 0 and off[-1] == col.n_elements
        rows += col.to_python()
        split = lambda flat: [flat[off[k]:off[k + 1]] for k in range(win.n_documents)]
        for dtype, acc in ((torch.int64, ints), (torch.float64, floats)):
            values, valid = col.numbers(dtype)
            assert values.dtype == dtype and valid.dtype == torch.bool and values.shape == valid.shape == (col.n_elements,)
            acc += split([v if ok else None for v, ok in zip(values.cpu().tolist(), valid.cpu().tolist())])
        s_off, s_bytes, s_valid = col.strings(bytes_capacity=1 if windows % 4 < 2 else None)
        assert s_off.shape == (col.n_elements + 1,) and s_valid.shape == (col.n_elements,)
        so, raw, ok = s_off.cpu().tolist(), s_bytes.cpu().numpy().tobytes(), s_valid.cpu().tolist()
        strings += split([raw[so[j]:so[j + 1]].decode("utf-8") if ok[j] else None for j in range(col.n_elements)])
        assert win.elements(0).fields.equal(col.fields) and win.elements("/id").n_elements == 0
        windows += 1
    assert windows >= 6 and len(rows) == len(lines)
    for k, (got, w) in enumerate(zip(rows, want)):
        assert (got is None) == (w is None) and (w is None or tsm.same_value(got, w)), (k, got, w)
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)
    for k, w in enumerate(want):
        items = w or []
        assert ints[k] == [v if is_int(v) else None for v in items], k
        assert floats[k] == [float(v) if is_int(v) or isinstance(v, float) else None for v in items], k
        assert strings[k] == [v if isinstance(v, str) else None for v in items], k
    assert rows[301] == ["first"] and rows[200] is None and rows[11] is None and rows[4] is None and rows[2] == [] and rows[1][1] == "e\né"
    assert sum(r is not None for r in rows) > 200
    plain = next(iter(DocumentStream(dev, tvd.upload(dev, data), len(data), window=4096, validate=True)))
    with pytest.raises(ValueError):
        plain.elements(0)
