"""A tape for every document of a window on the device (msj_tape_documents_device, csrc/tape_docs_kernel.hip).

Expected values come from the host twin of the same arithmetic (tests/tape_docs_math_host.cpp), which
tests/test_tape_documents_math.py holds against the one-document twin on every document's sub-arrays -- the definition in
include/msj_stage1.h -- and against Python's json.  Device output is compared with the twin word for word and byte for byte
over the WHOLE arrays (both start from the same fill, so a store the twin does not make shows, and so does one behind a
capacity: 64 bytes of canary behind each).  Token arrays come both ways, as in tests/test_tape.py: from the oracles, uploaded,
and from the real chain (shard, stage2_prep, documents, number_values, validate_documents).  A block is 1 024 tokens.
"""
import json

import numpy as np
import pytest

from tests import helpers
from tests import test_number_math as tnm
from tests import test_tape_documents_math as tdk
from tests import test_tape_math as ttm
from tests import test_validate_documents as tvd
from tests import test_validate_documents_math as tdm
from tests import test_validate_math as tvm

pytestmark = pytest.mark.gpu

BLOCK = 1024      # tokens per workgroup (csrc/tape_block.h: kBlock)
CANARY = 8        # tape words / records x 4 / 8 string bytes behind a capacity: 64 bytes each
MSJ_CAPACITY, BAD_ARGUMENT = 1, -1
RICH = b'{"k":[1,"a\\nb",{"z":null,"e":[]}],"s":"t\\u20ac","n":-2.5e3}'   # every kind of word; 28 tokens


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
def oracle():
    return helpers.load_oracle()


@pytest.fixture(scope="module")
def tm():
    return ttm.load_twin()


@pytest.fixture(scope="module")
def nm():
    return tnm.load_twin()


@pytest.fixture(scope="module")
def vtwin():
    return tdm.load_twin()


@pytest.fixture(scope="module")
def dtwin():
    return tdk.load_twin()


def to_device(dev, x):
    import torch

    x = np.ascontiguousarray(x)
    if x.dtype.fields is not None or x.dtype == np.uint64:
        x = x.view(np.int64)
    elif x.dtype == np.uint32:
        x = x.view(np.int32)
    return torch.from_numpy(x.copy()).to(dev.device)


class Uploaded:
    """The window's arrays from the oracles, uploaded: what the chain leaves on the device."""

    def __init__(self, dev, w, verdicts):
        from mojo_simdjson_amd import _lib

        pad = lambda a, dt: np.concatenate([np.ascontiguousarray(a, dtype=dt), np.zeros(8, dtype=dt)])   # (never an empty tensor)
        self.dev, self.length, self.n = dev, len(w.data), w.n
        self.d_buf = to_device(dev, np.frombuffer(w.data + b"\0" * 16, dtype=np.uint8))
        self.d_idx, self.d_match, self.d_end = (to_device(dev, pad(a, np.uint32)) for a in (w.idx, w.match, w.end))
        self.d_depth = to_device(dev, pad(w.depth, np.int32))
        self.d_type, self.d_flags = (to_device(dev, pad(a, np.uint8)) for a in (w.typ, w.flags))
        self.d_first = to_device(dev, pad(w.first, np.uint32))
        self.d_docs = to_device(dev, np.frombuffer(bytes(_lib.MsjDocumentsResult(*w.docs)), dtype=np.uint8))
        self.d_numbers = to_device(dev, np.concatenate([w.records, np.zeros(1, dtype=tdm.NUMBER_DTYPE)]))
        self.d_verdicts = to_device(dev, tdk.verdict_rows(verdicts)) if verdicts is not None else None


class FromChain:
    """The same arrays from the real chain on the device; verdicts: the rows of validate_documents, nothing waited for."""

    def __init__(self, dev, data, is_final, verdicts, max_depth=100, n=None, sync=True):
        c = tvd.Chain(dev, data, is_final=is_final, n=n, sync=sync)
        self.dev, self.length, self.n = dev, len(data), c.n
        self.d_buf, self.d_idx, self.d_type, self.d_depth, self.d_match, self.d_end, self.d_flags = \
            c.d_buf, c.d_idx, c.d_type, c.d_depth, c.d_match, c.d_end, c.d_flags
        self.d_first, self.d_docs, self.d_numbers = c.d_first, c.d_docs, c.d_numbers
        self.d_verdicts = c.verdicts(max_depth, sync=False)[0] if verdicts else None


def device_window(a, caps, strings=True, sync=True):
    """msj_tape_documents_device over the arrays `a` with the capacities `caps` (tdk.default_capacities), every output filled
    like the twin's and with its canary behind the capacity -> tdk.Built"""
    import torch
    from mojo_simdjson_amd import _lib

    dev, dv = a.dev, a.dev.device
    d_tape = torch.from_numpy(np.full(caps["tape_capacity"] + CANARY, tdk.TAPE_FILL, dtype=np.uint64).view(np.int64)).to(dv)
    d_sbuf = torch.full((caps["string_capacity"] + 8 * CANARY,), tdk.BYTE_FILL, dtype=torch.uint8, device=dv) if strings else None
    d_recs = torch.from_numpy(np.full((caps["capacity"] + CANARY) * 32, tdk.REC_FILL, dtype=np.uint8).view(np.int64).reshape(-1, 4)).to(dv)
    d_res, _, _, _ = dev.tape_documents(a.d_buf, a.length, a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end, a.d_flags, a.d_first,
                                        a.d_docs, a.d_numbers, caps["numbers_capacity"], d_verdicts=a.d_verdicts, d_tape=d_tape,
                                        tape_capacity=caps["tape_capacity"], d_string_buf=d_sbuf, string_capacity=caps["string_capacity"],
                                        strings=strings, d_doc_tapes=d_recs, capacity=caps["capacity"], sync=False)
    res = _lib.MsjTapeDocumentsResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
    recs = np.ascontiguousarray(d_recs.cpu().numpy()).view(tdk.DOC_TAPE_DTYPE).reshape(-1)
    return tdk.Built(res, d_tape.cpu().numpy().view(np.uint64), d_sbuf.cpu().numpy() if strings else None, recs, caps)


def same(got, want, where=None):
    """The device's result, records, words and bytes are the twin's, fill and canaries included"""
    assert got.summary() == want.summary(), (where, got.summary(), want.summary())
    assert got.canaries_intact(), where
    bad = np.nonzero(got.recs.view(np.uint8) != want.recs.view(np.uint8))[0]
    assert bad.size == 0, (where, "record", int(bad[0]) // 32, got.recs[int(bad[0]) // 32], want.recs[int(bad[0]) // 32])
    bad = np.nonzero(got.tape != want.tape)[0]
    assert bad.size == 0, (where, "word", int(bad[0]), hex(int(got.tape[bad[0]])), hex(int(want.tape[bad[0]])), bad.size)
    if want.sbuf is not None:
        bad = np.nonzero(got.sbuf != want.sbuf)[0]
        assert bad.size == 0, (where, "byte", int(bad[0]), bad.size)


def check(dev, oracle, nm, vtwin, dtwin, data, chain, verdicts=True, is_final=False, max_depth=100, strings=True, where=None, **caps):
    """One window on the device against the twin.  chain: the real chain, else the oracles' arrays uploaded; verdicts:
    d_verdicts given (the verdict twin's / the verdict call's), else NULL.  -> (WindowArrays, twin's Built, codes)"""
    w = tdm.WindowArrays(oracle, nm, data, is_final=is_final)
    rows = tdm.twin_documents(vtwin, w, max_depth)[0] if verdicts else None
    want = tdk.twin_window(dtwin, w, verdicts=rows, strings=strings, canary=CANARY, **caps)
    a = FromChain(dev, data, is_final, verdicts, max_depth) if chain else Uploaded(dev, w, rows)
    assert a.n == w.n, where
    same(device_window(a, want.caps, strings=strings), want, where)
    return w, want, [c for c, _ in rows] if rows else [0] * w.D


def test_corpus(dev, oracle, tm, nm, vtwin, dtwin):
    """The corpus of the CPU test: every stream both ways in, with d_verdicts given and with it NULL."""
    for j, (data, docs) in enumerate(tdk.corpus_streams()):
        for chain in (False, True):
            for verdicts in (False, True):
                w, want, _ = check(dev, oracle, nm, vtwin, dtwin, data, chain, verdicts=verdicts, where=(j, chain, verdicts))
                assert w.D == len(docs) == want.res.n_built
    data, docs = tdk.corpus_streams()[4]
    w, want, _ = check(dev, oracle, nm, vtwin, dtwin, data, True, strings=False)   # the layout-only form
    tdk.check_against_definition(tm, w, want, texts=docs)


def test_block_borders(dev, oracle, tm, nm, vtwin, dtwin):
    """A document that starts at token 1 023, 1 024 and 1 025 of the window, behind one-token and 7-token documents."""
    for at in (BLOCK - 1, BLOCK, BLOCK + 1):
        for ones_first in (True, False):
            head, k = tvd.filler(at, ones_first)
            tail, _ = tvd.filler(40, not ones_first)
            data = head + b"\n" + RICH + b" " + tail + b"\n"
            w, want, _ = check(dev, oracle, nm, vtwin, dtwin, data, chain=ones_first, where=(at, ones_first))
            assert int(w.first[k]) == at
            t0 = int(want.recs[k]["tape_first"])
            doc = tdk.Document(want.tape[t0:t0 + int(want.recs[k]["tape_words"])], want.sbuf[int(want.recs[k]["string_first"]):])
            assert doc.to_python() == json.loads(RICH.decode("utf-8"))


def test_flat_array_over_three_blocks(dev, oracle, tm, nm, vtwin, dtwin):
    """A flat array of 2 101 elements spanning three blocks (the pending count per block and td_span; its middle block
    holds no document start) with one-token documents on both sides: its count is exact."""
    elements = 2 * BLOCK + 53
    arr = b"[" + b"1," * (elements - 1) + b"1]"
    for lead in (3, 700):
        data = b" ".join([b'"x"'] * lead) + b" " + arr + b' true "y" 5 \n'
        w, want, _ = check(dev, oracle, nm, vtwin, dtwin, data, chain=lead == 3, where=lead)
        assert w.D == lead + 4 and 2 * elements > 3 * BLOCK + 1024
        t0 = int(want.recs[lead]["tape_first"])
        assert (int(want.tape[t0 + 1]) >> 32) & 0xFFFFFF == elements and int(want.tape[t0 + 1]) >> 56 == ord("[")
        tdk.check_against_definition(tm, w, want)


@pytest.mark.parametrize("kind", ["numbers", "strings", "atoms", "empties"])
def test_densest_blocks(dev, oracle, nm, vtwin, dtwin, kind):
    """4 096 one-token documents of each kind: the densest output per block (numbers: 4 words per token)."""
    docs = {"numbers": [b"%d" % k if k % 3 else b"-%d.5e3" % k for k in range(4096)], "strings": [b'"a"'] * 4096,
            "atoms": [b"true"] * 4096, "empties": [b"[]", b"{}"] * 2048}[kind]
    data = b"\n".join(docs) + b"\n"
    w, want, _ = check(dev, oracle, nm, vtwin, dtwin, data, chain=kind in ("numbers", "empties"), where=kind)
    assert w.D == 4096 == want.res.n_built
    per = {"numbers": 4, "strings": 3, "atoms": 3, "empties": 4}[kind]
    assert want.res.tape_words == per * 4096


def test_long_bodies(dev, oracle, tm, nm, vtwin, dtwin):
    """Bodies of 1 025 (the first a wave takes) and 70 000 bytes, escaped and plain, in a middle document, a few tokens in
    front of the next document's start in the same block: the base S(f_k) of the documents behind it."""
    for size in (1025, 70000):
        for escaped in (True, False):
            body = b"ab\\n\\\\\\u00e9" * (size // 12) if escaped else b"xy" * (size // 2)   # (whole escapes only)
            body += b"z" * (size - len(body))
            docs = [b'{"k":"v\\n"}'] * 5 + [b'["' + body + b'",1]', b'"t\\\\"', b'["s","\\u00e9"]', b'{"a":"b"}', b"2"]
            data = b"\n".join(docs) + b"\n"
            w, want, _ = check(dev, oracle, nm, vtwin, dtwin, data, chain=escaped, where=(size, escaped))
            assert w.D == 10 and int(w.first[9]) < BLOCK
            tdk.check_against_definition(tm, w, want, texts=docs)


def test_invalid_documents(dev, oracle, tm, nm, vtwin, dtwin):
    """One document of every error code between valid ones: its record has the code and zero sizes, its neighbours are
    exact.  A window whose first tokens sit below depth 0 in front of d_doc_first[0]."""
    valid = [doc for doc, _ in tvm.seeded_documents(20260, 64)]
    data, docs, bad = tdk.mixed_stream(valid)
    for md in (100, 3):
        for chain in (False, True):
            w, want, codes = check(dev, oracle, nm, vtwin, dtwin, data, chain, max_depth=md, where=(md, chain))
            assert all(codes[k] == c for k, c in bad.items() if c != tvm.DEPTH or md == 3)
            assert want.res.n_built == w.D - sum(1 for c in codes if c)
            tdk.check_against_definition(tm, w, want, codes=codes, texts=docs)
    check(dev, oracle, nm, vtwin, dtwin, data, True, verdicts=False)   # d_verdicts NULL: every slot is built, in bounds
    w, want, codes = check(dev, oracle, nm, vtwin, dtwin, tdk.BELOW_ZERO, chain=False, is_final=True)
    assert int(w.first[0]) == 2 and codes[0] == 0 and int(want.recs[0]["tape_first"]) == 0


def test_cut_window(dev, oracle, tm, nm, vtwin, dtwin):
    """A cut last document, not final: nothing at or past T is written, and the totals match.  No complete document, no
    token: a zero result."""
    docs = [RICH, b"[1.5,true]", b'"s"'] * 400   # T lies in the second block
    data = b" ".join(docs) + b' {"cut":[1,"abc'
    for chain in (False, True):
        w, want, _ = check(dev, oracle, nm, vtwin, dtwin, data, chain)
        assert (w.docs[0], w.D) == (1201, 1200) and BLOCK < w.T < w.n
        assert (want.tape[int(want.res.tape_words):] == tdk.TAPE_FILL).all()
    tdk.check_against_definition(tm, w, want, texts=docs)
    for data in (b'{"cut":[1,"abc', b"  \n "):
        for chain in (False, True):
            w, want, _ = check(dev, oracle, nm, vtwin, dtwin, data, chain)
            assert w.D == 0 and want.summary() == (0,) * 9


def test_capacities(dev, oracle, tm, nm, vtwin, dtwin):
    """Each of tape, string buffer, records and number records one short: MSJ_CAPACITY with the true sizes, the canaries
    intact; a second call with those sizes is exact."""
    data = b"\n".join([RICH, b"[1,2,3]", b'"abc"'] * 500) + b"\n"   # three blocks
    w, full, _ = check(dev, oracle, nm, vtwin, dtwin, data, True)
    exact = dict(tape_capacity=int(full.res.tape_words), string_capacity=int(full.res.string_bytes), numbers_capacity=int(full.res.n_numbers),
                 capacity=w.D)
    for name in exact:
        short = dict(exact)
        short[name] -= 1
        _, want, _ = check(dev, oracle, nm, vtwin, dtwin, data, chain=name in ("tape_capacity", "capacity"), where=name, **short)
        assert want.res.code == MSJ_CAPACITY
        sizes = dict(tape_capacity=int(want.res.tape_words), string_capacity=int(want.res.string_bytes),
                     numbers_capacity=int(want.res.n_numbers), capacity=int(want.res.n_documents))
        assert sizes == exact, name
        _, again, _ = check(dev, oracle, nm, vtwin, dtwin, data, True, where=(name, "again"), **sizes)
        assert again.res.code == 0
    tdk.check_against_definition(tm, w, again)


def test_bad_arguments(dev, oracle, nm, vtwin, dtwin):
    """Each is refused with nothing launched: the outputs keep what was in them."""
    import torch

    a = FromChain(dev, b'{"a":1} [1,2] "s" 3 ', False, True)
    sent = torch.full((8,), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    tape = torch.full((64,), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    sbuf = torch.full((64,), 0x5A, dtype=torch.uint8, device=dev.device)
    recs = torch.full((16, 4), tvd.SENTINEL, dtype=torch.int64, device=dev.device)

    def call(**kw):
        p = dict(buf=a.d_buf.data_ptr(), len=a.length, idx=a.d_idx.data_ptr(), n=a.n, typ=a.d_type.data_ptr(), dep=a.d_depth.data_ptr(),
                 mat=a.d_match.data_ptr(), end=a.d_end.data_ptr(), fl=a.d_flags.data_ptr(), first=a.d_first.data_ptr(),
                 docs=a.d_docs.data_ptr(), num=a.d_numbers.data_ptr(), ncap=a.n, nres=None, ver=a.d_verdicts.data_ptr(),
                 tape=tape.data_ptr(), tcap=64, sbuf=sbuf.data_ptr(), scap=64, recs=recs.data_ptr(), cap=16, res=sent.data_ptr())
        p.update(kw)
        return dev.lib.msj_tape_documents_device(dev.ctx, p["buf"], p["len"], p["idx"], p["n"], p["typ"], p["dep"], p["mat"], p["end"], p["fl"],
                                                 p["first"], p["docs"], p["num"], p["ncap"], p["nres"], p["ver"], p["tape"], p["tcap"],
                                                 p["sbuf"], p["scap"], p["recs"], p["cap"], p["res"], dev._stream())

    assert call(n=1 << 31) == MSJ_CAPACITY and call(len=(1 << 32) + 16) == MSJ_CAPACITY
    base = dict(idx=a.d_idx, dep=a.d_depth, mat=a.d_match, end=a.d_end, num=a.d_numbers, tape=tape, typ=a.d_type, fl=a.d_flags, docs=a.d_docs,
                ver=a.d_verdicts, recs=recs, first=a.d_first)
    for name, off in (("idx", 4), ("dep", 4), ("mat", 8), ("end", 4), ("num", 8), ("tape", 8), ("typ", 4), ("fl", 1), ("docs", 4), ("ver", 4),
                      ("recs", 4), ("first", 2)):
        assert call(**{name: base[name].data_ptr() + off}) == BAD_ARGUMENT, name
    assert call(res=sent.data_ptr() + 4) == BAD_ARGUMENT and call(nres=a.d_docs.data_ptr() + 4) == BAD_ARGUMENT
    for name in ("res", "docs", "first", "idx", "typ", "dep", "mat", "end", "fl", "buf", "tape", "recs", "num"):
        assert call(**{name: None}) == BAD_ARGUMENT, name
    torch.cuda.synchronize()
    assert all(bool((t == tvd.SENTINEL).all()) for t in (sent, tape, recs)) and bool((sbuf == 0x5A).all())
    assert call(sbuf=None, scap=0) == 0 and call(ver=None) == 0 and call() == 0
    # n == 0: a zero result whatever the split says
    assert call(n=0, idx=None, typ=None, dep=None, mat=None, end=None, fl=None, first=None, buf=None) == 0
    torch.cuda.synchronize()
    assert bool((sent == 0).all())


def test_chain_without_waiting(dev, oracle, nm, vtwin, dtwin):
    """Shard, prep, split, numbers, verdicts and tapes enqueued on one stream with nothing waited for (the token count from
    the oracle sizes the launches); one read at the end equals the twin."""
    data, docs, _ = tdk.mixed_stream([doc for doc, _ in tvm.seeded_documents(20260, 64)])
    data = data * 8   # two blocks
    w = tdm.WindowArrays(oracle, nm, data, is_final=False)
    rows = tdm.twin_documents(vtwin, w)[0]
    want = tdk.twin_window(dtwin, w, verdicts=rows, canary=CANARY)
    a = FromChain(dev, data, False, True, n=w.n, sync=False)
    same(device_window(a, want.caps), want)
    assert w.n > BLOCK and want.res.n_built == w.D - 8 * 6   # (DEPTH is no error at max_depth 100)


def ndjson_lines(total):
    """~total bytes of synthetic NDJSON: the statuses of one unit of mojo_simdjson_amd.synth, one per line (every other one
    with its non-ASCII characters as \\u escapes), each well inside a 4 KiB window"""
    from mojo_simdjson_amd import synth

    statuses = json.loads(synth.unit(total).tobytes().decode("utf-8"))["statuses"]
    return [json.dumps(s, separators=(",", ":"), ensure_ascii=bool(k % 2)).encode("utf-8") for k, s in enumerate(statuses)]


def test_document_stream_parse(dev):
    """~200 KiB of synthetic NDJSON through windows of 4 096 bytes (documents are cut and resumed), tiny initial capacities
    (the growth path runs): every Window.documents() entry equals json.loads of its line, an injected bad line gives None
    with its code; DocumentStream() and DocumentStream(validate=True) yield what they yield without parse."""
    from mojo_simdjson_amd.document_stream import DocumentStream

    lines = ndjson_lines(200 << 10)
    assert all(len(x) < 3000 for x in lines) and len(lines) > 100
    bad_at = len(lines) // 2
    lines[bad_at] = b'{"a":[1,2,tru]}'
    data = b"\n".join(lines) + b"\n"
    d_buf = tvd.upload(dev, data)
    stream = DocumentStream(dev, d_buf, len(data), window=4096, parse=True, tape_words=16, string_bytes=16, documents=1, numbers=1)
    got, shape, first_sizes = [], [], None
    for win in stream:
        if first_sizes is None:
            first_sizes = (stream._tape.numel(), stream._sbuf.numel(), stream._doc_tapes.shape[0], stream._numbers.shape[0])
        docs = win.documents()
        assert len(docs) == win.n_documents and win.n_built == sum(d is not None for d in docs) == win.n_documents - win.n_invalid
        assert win.document(0) is docs[0]
        codes = (win.d_verdicts.cpu().numpy()[:, 0] & 0xFFFFFFFF).tolist()
        recs = np.ascontiguousarray(win.d_doc_tapes.cpu().numpy()).view(tdk.DOC_TAPE_DTYPE).reshape(-1)
        assert recs["code"].tolist() == codes
        got += [(None, c) if d is None else (d.to_python(), 0) for d, c in zip(docs, codes)]
        shape.append((win.base, win.consumed, win.n_tokens, win.n_documents))
    assert all(now > was for now, was in zip(first_sizes, (16, 16, 1, 1))) and len(shape) > 40   # every array grew; many windows
    assert len(got) == len(lines)
    for k, (line, (value, code)) in enumerate(zip(lines, got)):
        if k == bad_at:
            assert (value, code) == (None, tvm.T_ATOM)
        else:
            assert code == 0 and value == json.loads(line.decode("utf-8")), k
    for kw in ({}, {"validate": True}):
        plain = list(DocumentStream(dev, d_buf, len(data), window=4096, **kw))
        assert [(p.base, p.consumed, p.n_tokens, p.n_documents) for p in plain] == shape
        for p in plain:
            assert (p.d_tape, p.d_string_buf, p.d_doc_tapes, p.n_built) == (None,) * 4
            assert (p.d_verdicts is None) == (not kw) and (p.n_invalid is None) == (not kw)
            with pytest.raises(ValueError):
                p.documents()
