"""A verdict for every document of a window on the device (msj_validate_documents_device, csrc/validate_docs_kernel.hip).

Always the real chain -- shard(is_final=False), stage2_prep(match=True), documents, number_values, validate_documents --
against the host twin of the same rule on the oracles' arrays (tests/validate_docs_math_host.cpp), which
tests/test_validate_documents_math.py holds against the one-document twin on every document's sub-arrays: the definition
in include/msj_stage1.h.  The corpus and its expected values are that file's, computed once.
"""
import numpy as np
import pytest

from tests import helpers
from tests import test_number_math as tnm
from tests import test_validate_documents_math as tdm
from tests import test_validate_math as tvm

pytestmark = pytest.mark.gpu

UINT64_MAX = tvm.UINT64_MAX
BLOCK = 1024  # tokens per workgroup of vd_tokens (csrc/validate_block.h: kBlock)
SENTINEL = 0x5A5A5A5A5A5A5A5A
CODES = {tvm.TAPE: b'{"a" 1}', tvm.DEPTH: b"[[[1]]]", tvm.STRING: b'["\\ud800x"]', tvm.T_ATOM: b"[tru]", tvm.F_ATOM: b"[fals]",
         tvm.N_ATOM: b"[nul,1]", tvm.NUMBER: b"[1,01]"}   # an invalid document of a few tokens per code (DEPTH: at max_depth 3)


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
def dtwin():
    return tdm.load_twin()


@pytest.fixture(scope="module")
def nm():
    return tnm.load_twin()


def upload(dev, data):
    import torch

    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev.device)


class Chain:
    """The calls in front of the verdict for one window.  records: number records asked for ("all": one per token, always
    enough); n: the token count if the caller knows it (nothing is read back then); sync=False: nothing is waited for."""

    def __init__(self, dev, data, is_final=False, records="all", n=None, sync=True):
        import torch

        self.dev, self.length = dev, len(data)
        self.d_buf = upload(dev, data)
        self.d_idx = torch.empty(len(data) + 3 + 4, dtype=torch.int32, device=dev.device)
        cin, self.cout = dev.new_carry(), dev.new_carry()
        dev.shard(self.d_buf, self.length, self.d_idx, cin, self.cout, is_final=False)
        self.n = int(dev.fetch(self.cout).count) if n is None else int(n)
        self.d_type, self.d_depth, _, self.d_match, self.d_end, self.d_flags = dev.stage2_prep(
            self.d_buf, self.length, self.d_idx, self.n, match=True, sync=sync)
        self.d_first, self.d_docs = dev.documents(self.d_buf, self.length, self.d_idx, self.n, self.d_type, self.d_depth,
                                                  is_final=is_final, d_carry=self.cout, sync=False)
        self.ncap = self.n if records == "all" else int(records)
        self.d_numbers, self.d_num = dev.number_values(self.d_buf, self.length, self.d_idx, self.n, self.d_flags, capacity=self.ncap,
                                                       sync=False)

    def verdicts(self, max_depth=100, numbers=True, capacity=None, sync=True):
        """-> ([(code, token)] per document the result counts, result); the rows behind them must be untouched.  sync=False:
        (d_verdicts, d_result), nothing waited for."""
        return device_verdicts(self, max_depth, numbers, capacity, sync)


def device_verdicts(a, max_depth=100, numbers=True, capacity=None, sync=True):
    """msj_validate_documents_device over the arrays `a` (a Chain, or the oracles' arrays uploaded with the number call's
    result: d_num, ncap), d_verdicts filled with SENTINEL and 8 rows longer than its capacity -> as Chain.verdicts"""
    import torch

    cap = a.n if capacity is None else int(capacity)
    rows = torch.full((cap + 8, 2), SENTINEL, dtype=torch.int64, device=a.dev.device)
    d_v, res = a.dev.validate_documents(a.d_buf, a.length, a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end, a.d_flags, a.d_first,
                                        a.d_docs, d_numbers=a.d_numbers, numbers_capacity=a.ncap,
                                        d_numbers_result=a.d_num if numbers else None, max_depth=max_depth, d_verdicts=rows, capacity=cap,
                                        sync=sync)
    if not sync:
        return d_v, res
    return unpack(rows, res) + (res,)


def unpack(rows, res):
    raw = rows.cpu().numpy()
    written = int(res.n_documents) if res.code == 0 else 0
    assert (raw[written:] == SENTINEL).all()   # d_verdicts[k] for k >= D is not written
    v = np.ascontiguousarray(raw[:written]).view(tdm.VERDICT_DTYPE).reshape(-1)
    assert (v["reserved"] == 0).all()
    return ([(int(c), int(t)) for c, t in zip(v["code"], v["error_token"])],)


def summary(res):
    return (res.code, res.flags, res.n_documents, res.n_invalid, res.first_invalid, res.n_escaped, res.reserved)


def check_window(dev, oracle, nm, dtwin, data, max_depths=(100,), is_final=False, where=None):
    """The chain on the device against the twin on the oracles' arrays.  -> (WindowArrays, {max_depth: verdicts})"""
    w = tdm.WindowArrays(oracle, nm, data, is_final=is_final)
    chain = Chain(dev, data, is_final=is_final)
    assert chain.n == w.n, where
    out = {}
    for md in max_depths:
        got, res = chain.verdicts(md)
        want, wres = tdm.twin_documents(dtwin, w, md)
        assert got == want, (where, md, [(k, g, x) for k, (g, x) in enumerate(zip(got, want)) if g != x][:5], data[:120])
        assert summary(res) == summary(wres), (where, md, summary(res), summary(wres))
        out[md] = got
    return w, out


def test_corpus(dev, oracle, nm, dtwin):
    """The corpus of the CPU test, stream by stream: every verdict, n_invalid, first_invalid and the flags equal the
    twin's; and the verdicts are the definition's (the one-document twin on the sub-arrays, computed once over there)."""
    hist = {}
    for (wf, want), data in zip(tdm.corpus_expected(), tdm.corpus_streams()[0]):
        w, got = check_window(dev, oracle, nm, dtwin, data, (100, 3))
        assert wf.D - 1 <= w.D <= wf.D   # a window is no end of a stream: a scalar that touches its end is cut
        for md in (100, 3):
            assert got[md] == want[md][:w.D], (data[:120], md)
            for c, _ in got[md]:
                hist[c] = hist.get(c, 0) + 1
    assert all(hist.get(c, 0) > 0 for c in (0, 3, 4, 5, 6, 7, 8, 9)), hist


def filler(tokens, ones_first):
    """Valid documents of one token and of 7 tokens, `tokens` tokens in all -> bytes"""
    sevens = max(0, (tokens - 20) // 7)
    ones = tokens - 7 * sevens
    parts = [b"1"] * ones + [b"[1,2,3]"] * sevens if ones_first else [b"[1,2,3]"] * sevens + [b"1"] * ones
    return b" ".join(parts), len(parts)


def test_block_borders(dev, oracle, nm, dtwin):
    """A document boundary on each token position from 5 in front of a block border to 5 behind it, an invalid document
    of each code planted there (it straddles the border, or starts right behind it); the other documents stay valid."""
    for at in range(BLOCK - 5, BLOCK + 6):
        for case, (code, doc) in enumerate(sorted(CODES.items())):
            head, k = filler(at, ones_first=(at + case) % 2 == 0)
            tail, _ = filler(40, ones_first=case % 2 == 1)
            data = head + b"\n" + doc + b" " + tail + b"\n"
            md = 3 if code == tvm.DEPTH else 100
            w, got = check_window(dev, oracle, nm, dtwin, data, (md,), where=(at, code))
            assert int(w.first[k]) == at, (at, code)
            assert [c for c, _ in got[md]] == [0] * k + [code] + [0] * (w.D - k - 1), (at, code)
            assert at <= got[md][k][1] < w.bounds(k)[1]


def test_blocks_without_a_start(dev, oracle, nm, dtwin):
    """A 3 001-token document between small ones: blocks in which no document starts.  An error in its middle, at its
    last token, and in the root bracket's partner (the first token's rule reads the last token from another block)."""
    ok = b"[" + b"1," * 1499 + b"1]"
    middle = b"[" + b"1," * 700 + b"tru," + b"1," * 798 + b"1]"
    last = b"[" + b"1," * 1499 + b"1,]"
    wrong_close = b"[" + b"1," * 1499 + b"1}"
    for name, doc, want in (("valid", ok, (0, UINT64_MAX)), ("middle", middle, (tvm.T_ATOM, 10 + 1 + 1400)),
                            ("last token", last, (tvm.TAPE, 10 + 3001)), ("root bracket", wrong_close, (tvm.TAPE, 10))):
        data = b"1 " * 10 + doc + b' {"a":1} 2 [3]\n'
        w, got = check_window(dev, oracle, nm, dtwin, data, where=name)
        assert w.D == 14 and got[100][10] == want, (name, got[100][10])
        assert [c for k, (c, _) in enumerate(got[100]) if k != 10] == [0] * 13


def test_one_token_documents(dev, oracle, nm, dtwin):
    """4 096 one-token documents, every other one `tru`: every odd document is T_ATOM."""
    data = b"1\ntru\n" * 2048
    w, got = check_window(dev, oracle, nm, dtwin, data)
    assert [c for c, _ in got[100]] == [0, tvm.T_ATOM] * 2048
    assert [t for c, t in got[100] if c] == list(range(1, 4096, 2))
    chain = Chain(dev, data)
    _, res = chain.verdicts()
    assert (res.n_documents, res.n_invalid, res.first_invalid) == (4096, 2048, 1)


def test_scope(dev, oracle, nm, dtwin):
    """The cut document is not judged and its verdict not written; too few verdicts; a window without a document."""
    data = b'{"a":1} [1,2] {"b":tru'
    w, got = check_window(dev, oracle, nm, dtwin, data)   # (unpack checks the rows behind D)
    assert (w.docs[0], w.D) == (3, 2) and got[100] == [(0, UINT64_MAX)] * 2
    w, got = check_window(dev, oracle, nm, dtwin, data + b"e} ", is_final=True)
    assert w.D == 3 and got[100] == [(0, UINT64_MAX)] * 3
    w, got = check_window(dev, oracle, nm, dtwin, data + b"} ", is_final=True)
    assert [c for c, _ in got[100]] == [0, 0, tvm.T_ATOM]
    chain = Chain(dev, b"1 2 3 4 ")
    got, res = chain.verdicts(capacity=3)
    assert res.code == tvm.CAPACITY and res.n_documents == 4 and got == []
    got, res = chain.verdicts(capacity=4)
    assert res.code == 0 and got == [(0, UINT64_MAX)] * 4
    w, got = check_window(dev, oracle, nm, dtwin, b"   \n \t ")
    assert w.n == 0 and got[100] == []
    _, res = Chain(dev, b"   \n \t ").verdicts()
    assert summary(res) == (0, 0, 0, 0, UINT64_MAX, 0, 0)


def test_numbers(dev, oracle, nm, dtwin):
    """Bad numbers in documents 3 and 70: NUMBER_ERROR with every record there; without them the flag, and nothing else."""
    docs = [b'{"k":%d,"v":[%d.5,-%de3]}' % (i, i, i) for i in range(100)]
    good = b"\n".join(docs) + b"\n"
    docs[3], docs[70] = b'{"k":01}', b"[1,[1e999]]"
    bad = b"\n".join(docs) + b"\n"
    w, got = check_window(dev, oracle, nm, dtwin, bad)
    assert [k for k, (c, _) in enumerate(got[100]) if c] == [3, 70] and got[100][3][0] == got[100][70][0] == tvm.NUMBER
    valid = [(0, UINT64_MAX)] * 100
    got, res = Chain(dev, bad, records=0).verdicts()
    assert got == valid and (res.flags, res.n_invalid) == (tvm.NUMBERS_UNCHECKED, 0)
    got, res = Chain(dev, bad, records=5).verdicts()      # some records are not all records
    assert got == valid and res.flags == tvm.NUMBERS_UNCHECKED
    got, res = Chain(dev, bad).verdicts(numbers=False)     # d_numbers_result NULL
    assert got == valid and res.flags == tvm.NUMBERS_UNCHECKED
    got, res = Chain(dev, good, records=0).verdicts()      # no bad number: no record is needed
    assert got == valid and res.flags == 0


def test_long_bodies(dev, oracle, nm, dtwin):
    """Escaped bodies for the lane (1 025 bytes is the first a wave takes), the wave and the grid, one bad escape near the
    end or none, as document 5 of 10."""
    for size in (1025, 70000, (1 << 20) + 4097):
        for bad in (True, False):
            body = b"ab\\n\\\\" * ((size - 40) // 6)   # whole escapes only: the one behind them stands on its own
            body += (b"\\q" if bad else b"\\t") + b"x" * (size - len(body) - 2)
            assert len(body) == size
            docs = [b'{"k":"v\\n"}'] * 5 + [b'["' + body + b'"]'] + [b'"t\\\\"', b"[1]", b'{"a":"\\u00e9"}', b"2"]
            w, got = check_window(dev, oracle, nm, dtwin, b"\n".join(docs) + b"\n", where=(size, bad))
            assert w.D == 10
            assert [c for c, _ in got[100]] == [0] * 5 + [tvm.STRING if bad else 0] + [0] * 4, (size, bad)
            if bad:
                assert got[100][5][1] == int(w.first[5]) + 1


def test_element_count(dev):
    """One array of 0xFFFFFF + 1 elements between two small documents: MSJ_CAPACITY at its closing bracket, for that
    document; with 0xFFFFFF elements nothing.  (Expected by hand: the oracles would take longer than the call.)"""
    for elements in (tvm.MAX_ELEMENTS + 1, tvm.MAX_ELEMENTS):
        arr = np.tile(np.frombuffer(b"0,", dtype=np.uint8), elements)
        arr[-1] = ord("]")
        data = b'{"a":1} [' + arr.tobytes() + b" [2]\n"
        chain = Chain(dev, data, records=0)
        assert chain.n == 5 + 2 * elements + 1 + 3
        got, res = chain.verdicts(capacity=16)
        close = 5 + 2 * elements   # '[' is token 5, then `elements` numbers and elements - 1 commas
        if elements > tvm.MAX_ELEMENTS:
            assert got == [(0, UINT64_MAX), (tvm.CAPACITY, close), (0, UINT64_MAX)]
            assert (res.code, res.flags, res.n_invalid, res.first_invalid) == (0, 0, 1, 1)
        else:
            assert got == [(0, UINT64_MAX)] * 3 and (res.code, res.flags, res.n_invalid) == (0, 0, 0)
        del chain


def test_document_stream_validate(dev, oracle, nm, dtwin, monkeypatch):
    """2 000 documents of the corpus through windows of 4 096 bytes (many documents are cut at window ends): the windows'
    verdicts, concatenated, are the twin's over the whole stream, error tokens compared as byte offsets.  Windows with a bad
    number take the number call twice.  validate=False: what the stream gave before, and none of the new fields."""
    from mojo_simdjson_amd.document_stream import DocumentStream

    data = b"\n".join(tdm.corpus_streams()[0][:32]) + b"\n"
    w = tdm.WindowArrays(oracle, nm, data, is_final=True)
    want, _ = tdm.twin_documents(dtwin, w)
    assert w.D >= 2000 and any(c == tvm.NUMBER for c, _ in want)
    want = [(c, None if c == 0 else (len(data) if t == w.n else int(w.idx[t]))) for c, t in want]
    d_buf = upload(dev, data)
    calls = []
    real = dev.number_values
    monkeypatch.setattr(dev, "number_values", lambda *a, **k: calls.append(k.get("capacity")) or real(*a, **k))
    got, shape, n_invalid = [], [], 0
    for win in DocumentStream(dev, d_buf, len(data), window=4096, validate=True):
        idx = win.d_idx.cpu().numpy().view(np.uint32)
        rows = np.ascontiguousarray(win.d_verdicts.cpu().numpy()).view(tdm.VERDICT_DTYPE).reshape(-1)
        assert rows.size == win.n_documents and win.verdict_flags == 0
        assert win.d_match.numel() == win.d_end.numel() == win.d_flags.numel() == win.n_tokens
        bad = [k for k in range(rows.size) if rows["code"][k]]
        assert win.n_invalid == len(bad) and win.first_invalid == (bad[0] if bad else None)
        for c, t in zip(rows["code"].tolist(), rows["error_token"].tolist()):
            got.append((c, None if c == 0 else win.base + (win.consumed if t == win.n_tokens else int(idx[t]))))
        shape.append((win.base, win.consumed, win.n_tokens, win.n_documents))
    assert got == want, [(k, g, x) for k, (g, x) in enumerate(zip(got, want)) if g != x][:5]
    assert len(shape) > 10 and len(calls) > len(shape) and any(c for c in calls)   # some windows asked for their records
    monkeypatch.undo()
    for kw in ({}, {"validate": False}):
        plain = list(DocumentStream(dev, d_buf, len(data), window=4096, **kw))
        assert [(p.base, p.consumed, p.n_tokens, p.n_documents) for p in plain] == shape
        for p in plain:
            assert (p.d_match, p.d_end, p.d_flags, p.d_verdicts, p.n_invalid, p.first_invalid, p.verdict_flags) == (None,) * 7


def test_bad_arguments(dev):
    """Nothing is launched on an argument error: the result keeps what was in it."""
    import torch

    chain = Chain(dev, b'{"a":1} [1,2] 3 ')
    sent = torch.full((7,), SENTINEL, dtype=torch.int64, device=dev.device)
    rows = torch.full((16, 2), SENTINEL, dtype=torch.int64, device=dev.device)

    def call(**kw):
        a = dict(buf=chain.d_buf.data_ptr(), len=chain.length, idx=chain.d_idx.data_ptr(), n=chain.n, typ=chain.d_type.data_ptr(),
                 dep=chain.d_depth.data_ptr(), mat=chain.d_match.data_ptr(), end=chain.d_end.data_ptr(), fl=chain.d_flags.data_ptr(),
                 first=chain.d_first.data_ptr(), docs=chain.d_docs.data_ptr(), num=chain.d_numbers.data_ptr(), ncap=chain.ncap,
                 nres=chain.d_num.data_ptr(), md=100, ver=rows.data_ptr(), cap=8, res=sent.data_ptr())
        a.update(kw)
        return dev.lib.msj_validate_documents_device(dev.ctx, a["buf"], a["len"], a["idx"], a["n"], a["typ"], a["dep"], a["mat"], a["end"],
                                                     a["fl"], a["first"], a["docs"], a["num"], a["ncap"], a["nres"], a["md"], a["ver"],
                                                     a["cap"], a["res"], dev._stream())

    bad, cap = -1, 1   # MSJ_ERR_BAD_ARGUMENT, MSJ_CAPACITY
    assert call(md=0) == bad
    assert call(n=1 << 31) == cap and call(len=(1 << 32) + 16) == cap
    for name, off in (("idx", 4), ("dep", 4), ("mat", 8), ("end", 4), ("num", 8), ("typ", 4), ("fl", 1), ("docs", 4), ("nres", 4),
                      ("ver", 4), ("first", 2)):
        base = dict(idx=chain.d_idx, dep=chain.d_depth, mat=chain.d_match, end=chain.d_end, num=chain.d_numbers, typ=chain.d_type,
                    fl=chain.d_flags, docs=chain.d_docs, nres=chain.d_num, ver=rows, first=chain.d_first)[name].data_ptr()
        assert call(**{name: base + off}) == bad, name
    assert call(res=sent.data_ptr() + 4) == bad
    assert call(res=None) == bad and call(docs=None) == bad and call(ver=None) == bad and call(first=None) == bad
    assert call(num=None) == bad   # numbers_capacity > 0 without records
    torch.cuda.synchronize()
    assert bool((sent == SENTINEL).all()) and bool((rows == SENTINEL).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((sent[:6] == SENTINEL).any())   # the 48 bytes of the result


def test_chain_without_waiting(dev, oracle, nm, dtwin):
    """The whole chain enqueued with nothing waited for (the token count from the oracle sizes the launches); one read at
    the end gives the same verdicts."""
    from mojo_simdjson_amd import _lib

    data = tdm.corpus_streams()[0][1]
    w = tdm.WindowArrays(oracle, nm, data, is_final=False)
    chain = Chain(dev, data, n=w.n, sync=False)
    rows, d_res = chain.verdicts(sync=False)
    res = _lib.MsjValidateDocumentsResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
    (got,) = unpack(rows, res)
    want, wres = tdm.twin_documents(dtwin, w)
    assert got == want and summary(res) == summary(wres)
