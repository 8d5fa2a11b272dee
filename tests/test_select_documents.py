"""Fields by path for every document of a window on the device (msj_select_documents_device, csrc/select_kernel.hip).

Expected values come from the host twin of the same arithmetic (tests/select_math_host.cpp), which
tests/test_select_math.py holds against the definition written in Python (tests/select_reference.py).  Device output is
compared with the twin over the WHOLE d_fields array (both start from the same fill, with 64 bytes of canary behind
n_paths * capacity records, so a store the twin does not make shows).  Token arrays come both ways, as in
tests/test_tape_documents.py: from the oracles, uploaded, and from the real chain (shard, stage2_prep, documents,
number_values, validate_documents); d_verdicts and d_numbers are given or NULL.  A block is 1 024 tokens.
"""
import json

import numpy as np
import pytest

from tests import helpers
from tests import select_reference as ref
from tests import test_number_math as tnm
from tests import test_select_math as tsm
from tests import test_tape_documents as ttd
from tests import test_tape_documents_math as tdk
from tests import test_validate_documents as tvd
from tests import test_validate_documents_math as tdm
from tests import test_validate_math as tvm

pytestmark = pytest.mark.gpu

BLOCK = 1024      # tokens per workgroup of sel_level (csrc/tape_block.h: kBlock)
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
    """The device, the oracles and the twins, and the compiled paths of every pointer list used so far"""
    return Env(dev)


class Env:
    def __init__(self, dev):
        self.dev, self.oracle, self.nm = dev, helpers.load_oracle(), tnm.load_twin()
        self.vtwin, self.stwin = tdm.load_twin(), tsm.load_twin()
        self._paths = {}

    def paths(self, pointers):
        key = tuple(pointers)
        if key not in self._paths:
            self._paths[key] = self.dev.compile_paths(pointers)
        return self._paths[key]


class Uploaded(ttd.Uploaded):
    """The window's arrays from the oracles, uploaded, with the number call's result"""

    def __init__(self, dev, w, verdicts):
        super().__init__(dev, w, verdicts)
        self.ncap = int(w.records.size)
        self.d_num = ttd.to_device(dev, np.frombuffer(bytes(w.numbers_result()), dtype=np.uint8))


class FromChain:
    """The same arrays from the real chain on the device; verdicts: the rows of validate_documents, nothing waited for"""

    def __init__(self, dev, data, is_final, verdicts, max_depth=100):
        c = tvd.Chain(dev, data, is_final=is_final)
        self.dev, self.length, self.n = dev, len(data), c.n
        self.d_buf, self.d_idx, self.d_type, self.d_depth, self.d_match, self.d_end, self.d_flags = \
            c.d_buf, c.d_idx, c.d_type, c.d_depth, c.d_match, c.d_end, c.d_flags
        self.d_first, self.d_docs, self.d_numbers, self.d_num, self.ncap = c.d_first, c.d_docs, c.d_numbers, c.d_num, c.ncap
        self.d_verdicts = c.verdicts(max_depth, sync=False)[0] if verdicts else None


def device_select(a, paths, capacity, numbers=True, numbers_result=True):
    """msj_select_documents_device over the arrays `a`, d_fields filled like the twin's with its canary -> tsm.Selected"""
    import torch
    from mojo_simdjson_amd import _lib

    dev = a.dev
    d_fields = torch.from_numpy(tsm.filled_fields(paths.n_paths, capacity).view(np.int64).reshape(-1, 2)).to(dev.device)
    d_res, _ = dev.select_documents(paths, a.d_buf, a.length, a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end, a.d_flags, a.d_first,
                                    a.d_docs, d_numbers=a.d_numbers if numbers else None, numbers_capacity=a.ncap if numbers else 0,
                                    d_numbers_result=a.d_num if numbers_result else None, d_verdicts=a.d_verdicts, d_fields=d_fields,
                                    capacity=capacity, sync=False)
    res = _lib.MsjSelectDocumentsResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
    fields = np.ascontiguousarray(d_fields.cpu().numpy()).view(tsm.FIELD_DTYPE).reshape(-1)
    return tsm.Selected(res, fields, paths.n_paths, capacity)


def same(got, want, where=None):
    """The device's result and every record are the twin's, fill and canary included"""
    assert got.summary() == want.summary(), (where, got.summary(), want.summary())
    bad = np.nonzero((got.fields.view(np.uint8) != want.fields.view(np.uint8)).reshape(-1, 16).any(axis=1))[0]
    if bad.size:
        j = int(bad[0])
        assert False, (where, "record", j // want.capacity, j % want.capacity, got.fields[j], want.fields[j], bad.size)


def check(env, data, pointers, chain, verdicts=True, numbers=True, numbers_result=True, is_final=False, max_depth=100, capacity=None,
          where=None, w=None):
    """One window on the device against the twin.  chain: the real chain, else the oracles' arrays uploaded; verdicts:
    d_verdicts given (the verdict twin's / the verdict call's), else NULL.  -> (WindowArrays, twin's Selected, codes)"""
    w = tdm.WindowArrays(env.oracle, env.nm, data, is_final=is_final) if w is None else w
    rows = tdm.twin_documents(env.vtwin, w, max_depth)[0] if verdicts else None
    want = tsm.twin_select(env.stwin, w, pointers, verdicts=rows, numbers=numbers, numbers_result=numbers_result, capacity=capacity)
    a = FromChain(env.dev, data, is_final, verdicts, max_depth) if chain else Uploaded(env.dev, w, rows)
    assert a.n == w.n, where
    same(device_select(a, env.paths(pointers), want.capacity, numbers, numbers_result), want, where)
    return w, want, [c for c, _ in rows] if rows else [0] * w.D


def pad(elements):
    """An array of `elements` zeros: 2 * elements + 1 tokens"""
    return b"[" + b",".join([b"0"] * elements) + b"]"


def test_corpus_and_pins(env):
    """The corpus and the pins of the CPU test, one window each: both ways in, d_verdicts given and NULL, d_numbers given
    and NULL (and with the records but without the number call's result)."""
    streams = [tsm.pin_stream()] + tsm.corpus()
    for j, (data, docs, pointers) in enumerate(streams):
        w = tdm.WindowArrays(env.oracle, env.nm, data, is_final=False)
        for v, (chain, verdicts) in enumerate(((False, False), (False, True), (True, False), (True, True))):
            numbers, nres = (j + v) % 3 != 0, (j + v) % 5 != 1
            _, want, _ = check(env, data, pointers, chain, verdicts=verdicts, numbers=numbers, numbers_result=nres, w=w, where=(j, v))
        assert w.D == len(docs)
        if j < 6:
            tsm.check_against_reference(w, want, pointers, docs, bits=False)


def test_block_borders(env):
    """A matching key on every token position from 3 in front of a block border to 3 behind it -- the key, its ':' and its
    value fall into different blocks -- and the same with the document's start moved across the border."""
    pointers = ["/k", "/k/q", "/a", "", "/k/a"]
    for doc, lead in ((b'{"k":{"q":7},"a":1}', 1), (b'{"a":[1,2],"b":2,"k":{"q":"v"}}', 0)):
        for at in range(BLOCK - 3, BLOCK + 4):
            head, k = tvd.filler(at - lead, at % 2 == 0)
            tail, _ = tvd.filler(30, at % 2 == 1)
            data = head + b"\n" + doc + b" " + tail + b"\n"
            w, want, _ = check(env, data, pointers, chain=at % 2 == 0, numbers=at % 3 != 0, where=(doc, at))
            assert int(w.first[k]) == at - lead
            col = lambda p: tsm.field_value(want.column(p)[k], np.frombuffer(w.data, dtype=np.uint8), w.idx, w.end)
            assert col(1) == json.loads(doc)["k"]["q"] and col(0) == json.loads(doc)["k"] and int(want.column(4)[k]["code"]) == 20
            if lead:
                assert int(want.column(0)[k]["token"]) == at + 2 and w.data[int(w.idx[at])] == ord('"')


def test_first_duplicate_wins_across_blocks(env):
    """Two duplicate keys in different blocks, flat and one level down: the first one wins, whichever block reports first."""
    doc = b'{"k":1,"o":{"d":"first","p":' + pad(600) + b',"d":"second"},"p":' + pad(600) + b',"k":2}'
    pointers = ["/k", "/o/d", "/p", "/o/p"]
    for lead in (5, 900):
        data = b" ".join([b"1"] * lead) + b" " + doc + b' {"k":3}\n'
        w, want, _ = check(env, data, pointers, chain=lead == 5, where=lead)
        assert w.T > 2 * BLOCK
        out = tsm.check_against_reference(w, want, pointers, [b"1"] * lead + [doc, b'{"k":3}'])
        assert out[(0, lead)] == (0, 1) and out[(1, lead)] == (0, "first") and out[(0, lead + 1)] == (0, 3)


def test_long_document_and_blocks_without_a_start(env):
    """A document of about 3 000 tokens whose key lies in its third block (no document starts in its second and third),
    between short ones."""
    doc = b'{"p":' + pad(1400) + b',"k":{"deep":true,"n":-1.5}}'
    docs = [b'{"k":{"deep":1}}', b"[1]", doc, b'{"k":{"n":2}}', b'"k"']
    pointers = ["/k/deep", "/k/n", "/k", "/p/k"]
    data = tdk.join(docs, b"\n")
    for chain in (False, True):
        w, want, _ = check(env, data, pointers, chain)
        f, e = w.bounds(2)
        assert e - f > 2800 and int(want.column(0)[2]["token"]) - f > 2 * BLOCK
    out = tsm.check_against_reference(w, want, pointers, docs)
    assert [out[(0, k)] for k in range(5)] == [(0, 1), (17, None), (0, True), (20, None), (17, None)] and out[(1, 2)] == (0, -1.5)


def test_one_token_documents(env):
    """4 096 one-token documents with the path "" and with the path /a: a record per document, no key anywhere."""
    docs = [b"%d" % k if k % 3 else b'"s%d"' % k for k in range(4096)]
    data = b"\n".join(docs) + b"\n"
    for chain, pointers in ((True, [""]), (False, ["/a"]), (True, ["/a", ""])):
        w, want, _ = check(env, data, pointers, chain, where=pointers)
        assert w.D == 4096 and want.res.n_found == 4096 * pointers.count("")
    tsm.check_against_reference(w, want, pointers, docs)


def test_eight_levels_in_eight_blocks(env):
    """An 8-segment path through eight nested objects, each level's key in another block; its prefixes as paths of their own
    (the same pass serves them), and a path that leaves it one level down."""
    doc, keys = b'"bottom"', ["l%d" % k for k in range(8)]
    for k in reversed(keys):
        doc = b'{"p":' + pad(520) + b',"' + k.encode() + b'":' + doc + b"}"
    pointers = [ref.pointer_of(keys[:n]) for n in (8, 1, 4, 7)] + ["/l0/l1/x/l3", "/l0/p/l2", ref.pointer_of(keys[:7] + ["p"]), "/l0/l1/l2/l3/l4/l5/l6/l7x"]
    data = b'{"l0":1} ' + doc + b' {"l0":{"l1":{"l2":{"l3":{"l4":{"l5":{"l6":{"l7":8}}}}}}}}\n'
    for chain in (False, True):
        w, want, _ = check(env, data, pointers, chain)
    tokens = [int(want.column(p)[1]["token"]) for p in (1, 2, 3, 0)]
    assert sorted({t // BLOCK for t in tokens}) == [1, 4, 7, 8]
    out = tsm.check_against_reference(w, want, pointers, [b'{"l0":1}', doc, data.split(b" ")[-1].strip()])
    assert out[(0, 1)] == (0, "bottom") and out[(0, 2)] == (0, 8) and out[(0, 0)] == (17, None)
    assert [out[(p, 1)][0] for p in (4, 5, 7)] == [20, 17, 20] and out[(6, 1)] == (0, [0] * 520)


def test_sixteen_paths(env):
    """16 paths at once, two of them equal and two sharing a prefix, over the pins and over a seeded stream."""
    pointers = tsm.PIN_PATHS + ["/a", "/a/b/c", "/x", "/x/a", "/0", "/ab/zz", "/no", "/a~1b/x"]
    assert len(pointers) == 16 and pointers.count("/a") == 2
    data, docs, _ = tsm.pin_stream()
    w, want, _ = check(env, data, pointers, True)
    out = tsm.check_against_reference(w, want, pointers, docs)
    assert np.array_equal(want.column(0), want.column(8)) and out[(11, 1)] == (0, 1)
    data, docs, drawn = tsm.corpus()[7]
    pointers = (drawn + [drawn[1], drawn[2]] * 8)[:16]
    w, want, _ = check(env, data, pointers, False)
    tsm.check_against_reference(w, want, pointers, docs)


def test_longest_escaped_key(env):
    """An escaped key of 1 530 raw bytes (255 x \\u0061) that matches, and one that differs in its last escape."""
    key = b"\\u0061" * 255
    docs = [b'{"' + key[:-1] + b'2":0,"' + key + b'":1}', b'{"' + key[:-1] + b'2":2}', b'{"' + b"a" * 255 + b'":3}']
    pointers = ["/" + "a" * 255, "/" + "a" * 254 + "b", "/" + "a" * 254]
    for chain in (False, True):
        w, want, _ = check(env, tdk.join(docs, b" "), pointers, chain)
    out = tsm.check_against_reference(w, want, pointers, docs)
    assert [out[(0, k)] for k in range(3)] == [(0, 1), (20, None), (0, 3)] and [out[(1, k)] for k in range(3)] == [(0, 0), (0, 2), (20, None)]


def test_invalid_document_across_a_border(env):
    """A document with a verdict code straddling a block border between two valid ones, for every code: its records have
    the code, its neighbours' are exact; the same window without verdicts stays in bounds."""
    pointers = ["/a", "", "/a/b", "/b"]
    for case, (code, bad) in enumerate(sorted(tvd.CODES.items())):
        head, k = tvd.filler(BLOCK - 2 - 17, case % 2 == 0)   # (the left neighbour has 17 tokens: the bad one starts at 1 022)
        docs = [b'{"b":{"a":1},"a":{"b":"left"}}', bad, b'{"a":{"b":"right"}}']
        data = head + b" " + b" ".join(docs) + b" 1 \n"
        for chain in (False, True):
            w, want, codes = check(env, data, pointers, chain, max_depth=3, where=(code, chain))
            assert codes[k + 1] == code and codes[k] == codes[k + 2] == 0 and int(w.first[k + 1]) <= BLOCK < int(w.first[k + 2])
            assert want.column(2)[k:k + 3]["code"].tolist() == [0, code, 0]
        check(env, data, pointers, True, verdicts=False, max_depth=3, where=(code, "free"))


def test_capacity(env):
    """D > capacity: MSJ_CAPACITY, n_documents = D, no record written and the canary intact; with room for D the call is exact."""
    data, docs, pointers = tsm.corpus()[9]
    w = tdm.WindowArrays(env.oracle, env.nm, data, is_final=False)
    for chain in (False, True):
        _, want, _ = check(env, data, pointers, chain, capacity=w.D - 1, w=w)
        assert want.summary() == (MSJ_CAPACITY, 0, w.D, len(pointers), 0, 0, 0) and want.untouched(0)
        _, want, _ = check(env, data, pointers, chain, capacity=w.D, w=w)
        assert want.res.code == 0
    for empty in (b'{"cut":[1,"abc', b"  \n "):
        w0, want, _ = check(env, empty, pointers, True)
        assert w0.D == 0 and want.summary() == (0, 0, 0, len(pointers), 0, 0, 0)


def test_bad_arguments(env):
    """Each is refused with nothing launched: the outputs keep what was in them."""
    import torch

    dev = env.dev
    a = FromChain(dev, b'{"a":1} [1,2] "s" 3 ', False, True)
    paths = env.paths(["/a", ""])
    sent = torch.full((8,), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    recs = torch.full((2 * 16 + 4, 2), tvd.SENTINEL, dtype=torch.int64, device=dev.device)

    def call(**kw):
        p = dict(paths=paths.handle, buf=a.d_buf.data_ptr(), len=a.length, idx=a.d_idx.data_ptr(), n=a.n, typ=a.d_type.data_ptr(),
                 dep=a.d_depth.data_ptr(), mat=a.d_match.data_ptr(), end=a.d_end.data_ptr(), fl=a.d_flags.data_ptr(),
                 first=a.d_first.data_ptr(), docs=a.d_docs.data_ptr(), num=a.d_numbers.data_ptr(), ncap=a.ncap, nres=a.d_num.data_ptr(),
                 ver=a.d_verdicts.data_ptr(), recs=recs.data_ptr(), cap=16, res=sent.data_ptr())
        p.update(kw)
        return dev.lib.msj_select_documents_device(dev.ctx, p["paths"], p["buf"], p["len"], p["idx"], p["n"], p["typ"], p["dep"], p["mat"],
                                                   p["end"], p["fl"], p["first"], p["docs"], p["num"], p["ncap"], p["nres"], p["ver"],
                                                   p["recs"], p["cap"], p["res"], dev._stream())

    assert call(n=1 << 31) == MSJ_CAPACITY and call(len=(1 << 32) + 16) == MSJ_CAPACITY
    base = dict(idx=a.d_idx, dep=a.d_depth, mat=a.d_match, end=a.d_end, num=a.d_numbers, recs=recs, typ=a.d_type, fl=a.d_flags, docs=a.d_docs,
                ver=a.d_verdicts, nres=a.d_num, res=sent, first=a.d_first)
    for name, off in (("idx", 4), ("dep", 4), ("mat", 8), ("end", 4), ("num", 8), ("recs", 8), ("typ", 4), ("fl", 1), ("docs", 4), ("ver", 4),
                      ("nres", 4), ("res", 4), ("first", 2)):
        assert call(**{name: base[name].data_ptr() + off}) == BAD_ARGUMENT, name
    for name in ("paths", "res", "docs", "first", "idx", "typ", "dep", "mat", "end", "fl", "buf", "recs", "num"):
        assert call(**{name: None}) == BAD_ARGUMENT, name
    torch.cuda.synchronize()
    assert bool((sent == tvd.SENTINEL).all()) and bool((recs == tvd.SENTINEL).all())
    assert call(num=None, ncap=0) == 0 and call(ver=None) == 0 and call(nres=None) == 0 and call() == 0
    # n == 0: a zero result whatever the split says
    assert call(n=0, idx=None, typ=None, dep=None, mat=None, end=None, fl=None, first=None, buf=None) == 0
    torch.cuda.synchronize()
    assert sent.cpu().numpy()[:6].tolist() == [0, 0, 2, 0, 0, 0]
    with pytest.raises(ValueError):
        dev.compile_paths(["/a", "b"])
    for beyond in ([], ["/a"] * 17, ["/" + "k" * 256], ["/1/2/3/4/5/6/7/8/9"]):
        with pytest.raises(ValueError):
            dev.compile_paths(beyond)


def test_document_stream_select(env):
    """~200 documents through windows of 4 096 bytes (documents are cut and resumed): Window.values(p) equals the reference
    per document, an injected bad line gives None with its code, n_found equals the host count; a stream forced to grow
    d_fields (documents=1) gives the same.  Without select, column / values raise."""
    from mojo_simdjson_amd.document_stream import DocumentStream

    dev = env.dev
    lines = ttd.ndjson_lines(200 << 10)[:200]
    bad_at = len(lines) // 2
    lines[bad_at] = b'{"id":1,"a":[1,2,tru]}'
    lines[3] = b'{"id":"dup","id":2,"user":7}'
    data = b"\n".join(lines) + b"\n"
    decoded = [None if k == bad_at else ref.decode(x) for k, x in enumerate(lines)]
    chains = sorted({c for d in decoded[:20] if d is not None for c in ref.key_paths(d) if tsm.usable(c)}, key=lambda c: (len(c), c))
    pointers = ["/id", "/user/name", "", "/user", "/no"] + [ref.pointer_of(c) for c in chains[-3:]]
    d_buf = tvd.upload(dev, data)
    runs = []
    for kw in ({}, {"documents": 1, "numbers": 1}):
        stream = DocumentStream(dev, d_buf, len(data), window=4096, select=pointers, **kw)
        got, windows, cut = [[] for _ in pointers], 0, 0
        for win in stream:
            cols = [win.column(p) for p in range(len(pointers))]
            assert all(c.shape == (win.n_documents,) for c in cols) and win.d_fields.shape == (len(pointers), win.n_documents, 2)
            assert win.n_found == sum(int((c["code"] == 0).sum()) for c in cols)
            assert win.values("/id") == win.values(0)
            for p in range(len(pointers)):
                got[p] += list(zip(cols[p]["code"].tolist(), win.values(p)))
            windows += 1
            cut += win.consumed < win.length
        assert windows >= 4 and cut >= 1 and len(got[0]) == len(lines)
        runs.append(got)
        for p, pointer in enumerate(pointers):
            for k, (code, value) in enumerate(got[p]):
                want = (tvm.T_ATOM, None) if k == bad_at else ref.lookup(decoded[k], pointer)
                assert code == want[0] and tsm.same_value(value, want[1]), (pointer, k, code, value, want)
    assert runs[0] == runs[1] and runs[0][0][3] == (0, "dup")
    assert stream._fields.shape[1] > 1 and stream._numbers.shape[0] > 1   # both grew
    plain = next(iter(DocumentStream(dev, d_buf, len(data), window=4096, validate=True)))
    assert plain.d_fields is None and plain.n_found is None
    for call in (plain.column, plain.values):
        with pytest.raises(ValueError):
            call(0)
