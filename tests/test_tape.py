"""The document's tape and string buffer on the device (msj_tape_device, csrc/tape_kernel.hip) through the C ABI.

Expected values come from the host twin of the same arithmetic (tests/tape_math_host.cpp), which tests/test_tape_math.py
holds against a serial tape builder and against Python's json on this corpus.  Device output is compared with the twin word
for word and byte for byte.  Two ways in, as in tests/test_validate.py: the real chain on the device (parse_document), and
token arrays built on the host by the oracles, uploaded together, one call per document on one stream with nothing waited
for in between.  DERIVED like the token arrays: the definition is include/msj_stage1.h's.
"""
import ctypes
import json

import numpy as np
import pytest

from tests import helpers
from tests import test_number_math as tnm
from tests import test_tape_math as ttm
from tests import test_validate_math as tvm

pytestmark = pytest.mark.gpu

BLOCK = 1024      # tokens per workgroup of tape_sums / tape_pos / tape_emit (csrc/tape_kernel.hip: kBlock)
LANE_BODY = 1024  # bodies up to this many bytes are handled by their lane, longer ones by a wave (kLaneBody)
CANARY = 64       # bytes behind every capacity
MSJ_CAPACITY = 1


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
def tm():
    return ttm.load_twin()


@pytest.fixture(scope="module")
def nm():
    return tnm.load_twin()


def up16(x):
    return (x + 15) & ~15


def run_batch(dev, tm, items, strings=True, verdict_code=None, compare=True):
    """items: (data, host arrays, capacities) per document; capacities: dict with any of tape_capacity / string_capacity /
    numbers_capacity (default: the bounds n + numbers + 2 and 5 * len // 3 + 64, every record).  All arrays in one upload
    (every slice on the 16-byte grid), one msj_tape_device per document on one stream with nothing waited for, the outputs
    read once.  Each result, the tape up to its capacity and the string buffer up to its capacity equal the twin's, and the
    CANARY bytes behind each capacity are untouched.  verdict_code: every call gets a d_verdict with that code.
    -> list of (MsjTapeResult, tape uint64[min(words, capacity)], string bytes)"""
    import torch
    from mojo_simdjson_amd import _lib

    place = []
    t = b = k = tw = sb = 0
    for data, a, caps in items:
        n, nn = len(a["idx"]), a["bits"].size
        tcap = caps.get("tape_capacity", n + nn + 2)
        scap = caps.get("string_capacity", 5 * len(data) // 3 + 64) if strings else 0
        ncap = caps.get("numbers_capacity", nn)
        place.append((b, t, n, k, nn, tw, tcap, sb, scap, ncap))
        b += len(data)
        t += up16(n)
        k += nn
        tw += up16(tcap + CANARY // 8)
        sb += up16(scap + CANARY)
    h_buf = np.zeros(max(b, 1), dtype=np.uint8)
    h_idx, h_match, h_end = (np.zeros(max(t, 1), dtype=np.uint32) for _ in range(3))
    h_depth = np.zeros(max(t, 1), dtype=np.int32)
    h_type, h_flags = (np.zeros(max(t, 1), dtype=np.uint8) for _ in range(2))
    h_num = np.zeros((max(k, 1), 2), dtype=np.uint64)
    for (data, a, _), (b0, t0, n, k0, nn, *_) in zip(items, place):
        h_buf[b0:b0 + len(data)] = np.frombuffer(data, dtype=np.uint8)
        h_idx[t0:t0 + n], h_type[t0:t0 + n], h_depth[t0:t0 + n] = a["idx"], a["typ"], a["depth"]
        h_match[t0:t0 + n], h_end[t0:t0 + n], h_flags[t0:t0 + n] = a["match"], a["end"], a["flags"]
        h_num[k0:k0 + nn, 0] = a["bits"]
        h_num[k0:k0 + nn, 1] = a["num_tokens"].astype(np.uint64) | (a["kinds"].astype(np.uint64) << np.uint64(32))
    dv = dev.device

    def up(x):
        return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else (x.view(np.int64) if x.dtype == np.uint64 else x)).to(dv)

    d_buf, d_idx, d_type, d_depth, d_match, d_end, d_flags, d_num = (up(x) for x in (h_buf, h_idx, h_type, h_depth, h_match, h_end, h_flags, h_num))
    d_tape = torch.full((max(tw, 2),), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dv)
    d_sbuf = torch.full((max(sb, 16),), 0x5A, dtype=torch.uint8, device=dv)
    d_res = torch.full((len(items), 32), 0xAB, dtype=torch.uint8, device=dv)
    d_verdict = None
    if verdict_code is not None:
        v = _lib.MsjValidateResult()
        v.code, v.error_token, v.error_offset = verdict_code, 0, 0
        d_verdict = torch.from_numpy(np.frombuffer(bytes(v), dtype=np.uint8).copy()).to(dv)
    stream = dev._stream()
    for j, ((data, _, _), (b0, t0, n, k0, nn, tw0, tcap, sb0, scap, ncap)) in enumerate(zip(items, place)):
        rc = dev.lib.msj_tape_device(dev.ctx, d_buf.data_ptr() + b0, len(data), d_idx.data_ptr() + 4 * t0, n, d_type.data_ptr() + t0,
                                     d_depth.data_ptr() + 4 * t0, d_match.data_ptr() + 4 * t0, d_end.data_ptr() + 4 * t0,
                                     d_flags.data_ptr() + t0, d_num.data_ptr() + 16 * k0, ncap, None,
                                     d_verdict.data_ptr() if d_verdict is not None else None, d_tape.data_ptr() + 8 * tw0, tcap,
                                     (d_sbuf.data_ptr() + sb0) if strings else None, scap, d_res.data_ptr() + 32 * j, stream)
        assert rc == 0, rc
    raw = d_res.cpu().numpy().tobytes()
    g_tape = d_tape.cpu().numpy().view(np.uint64)
    g_sbuf = d_sbuf.cpu().numpy()
    out = []
    for j, ((data, a, _), (b0, t0, n, k0, nn, tw0, tcap, sb0, scap, ncap)) in enumerate(zip(items, place)):
        got = _lib.MsjTapeResult.from_buffer_copy(raw[32 * j:32 * j + 32])
        mine_t, mine_s = g_tape[tw0:tw0 + tcap + CANARY // 8], g_sbuf[sb0:sb0 + scap + CANARY]
        assert (mine_t[tcap:] == 0x5A5A5A5A5A5A5A5A).all(), (j, "tape canary")
        assert (mine_s[scap:] == 0x5A).all(), (j, "string canary")
        if verdict_code:
            assert (got.code, got.flags, got.tape_words, got.string_bytes, got.n_strings) == (verdict_code, 0, 0, 0, 0)
            assert (mine_t == 0x5A5A5A5A5A5A5A5A).all() and (mine_s == 0x5A).all()  # only d_result is written
            out.append((got, None, None))
            continue
        if not compare:
            out.append((got, None, None))
            continue
        want, w_tape, w_sbuf = ttm.twin_build(tm, data, a, tape_capacity=tcap, string_capacity=scap, numbers_capacity=ncap, strings=strings)
        quint = lambda r: (r.code, r.flags, r.tape_words, r.string_bytes, r.n_strings)
        assert quint(got) == quint(want), (j, data[:120], quint(got), quint(want))
        used_t = min(int(want.tape_words), tcap)
        bad = np.nonzero(mine_t[:used_t] != w_tape[:used_t])[0]
        assert bad.size == 0, (j, data[:120], int(bad[0]), hex(int(mine_t[bad[0]])), hex(int(w_tape[bad[0]])), bad.size)
        used_s = min(int(want.string_bytes), scap) if strings else 0
        if strings:
            bad = np.nonzero(mine_s[:used_s] != w_sbuf[:used_s])[0]
            assert bad.size == 0, (j, data[:120], int(bad[0]), bad.size)
        out.append((got, mine_t[:used_t].copy(), mine_s[:used_s].copy()))
    return out


def arrays_of(oracle, nm, data):
    a = ttm.host_arrays(oracle, nm, data)
    assert not isinstance(a, int), (a, data[:120])
    return a


def device_document(dev, data, max_depth=100, exact_strings=False):
    import torch

    d_buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev.device)
    return dev.parse_document(d_buf, len(data), max_depth, exact_strings=exact_strings)


def check_chain(dev, oracle, tm, nm, data, max_depth=100, exact_strings=False):
    """parse_document on the device against the twin on the oracles' arrays -> Document"""
    from mojo_simdjson_amd.document import Document

    got = device_document(dev, data, max_depth, exact_strings)
    assert not isinstance(got, int), got
    verdict, tres, d_tape, d_sbuf = got
    assert (verdict.code, verdict.flags) == (0, 0), (verdict.code, verdict.flags, data[:120])
    a = arrays_of(oracle, nm, data)
    want, w_tape, w_sbuf = ttm.twin_build(tm, data, a)
    assert (tres.code, tres.flags, tres.tape_words, tres.string_bytes, tres.n_strings) == \
        (0, 0, want.tape_words, want.string_bytes, want.n_strings), data[:120]
    doc = Document.from_device(tres, d_tape, d_sbuf)
    assert np.array_equal(doc.tape, w_tape[:want.tape_words]), data[:120]
    assert np.array_equal(doc.string_buf, w_sbuf[:want.string_bytes]), data[:120]
    if exact_strings:
        assert d_sbuf.numel() == max(int(want.string_bytes), 1)
    return doc


def test_valid_corpus_batched(dev, oracle, tm, nm):
    """The valid documents of tests/test_tape_math.py's corpus through host-built arrays: every word and byte equal to the
    twin's; every other chunk in the layout-only form."""
    items, total = [], 0
    flip = [True]

    def flush():
        run_batch(dev, tm, items, strings=flip[0])
        flip[0] = not flip[0]
        items.clear()

    for _, doc in ttm.valid_corpus(oracle):
        items.append((doc, arrays_of(oracle, nm, doc), {}))
        total += 1
        if len(items) >= 20000:
            flush()
    if items:
        flush()
    assert total >= 200000


def test_chain_fixtures_and_seeded(dev, oracle, tm, nm):
    """The four stage-2 fixtures of the reference and 1 000 seeded documents through the real chain (parse_document)."""
    for js in ttm.fixture_documents():
        doc = check_chain(dev, oracle, tm, nm, js)
        assert doc.to_python() == json.loads(js.decode("utf-8"))
        text, ok = doc.dump_raw_tape()
        assert ok and text.startswith("0 : 114\t// pointing to %d (right after last node)\n" % doc.tape.size)
        assert text.endswith("%d : 114\t// pointing to 0 (start root)\n" % (doc.tape.size - 1))
    for k, (text, _) in enumerate(tvm.seeded_documents(20260, 1000)):
        doc = check_chain(dev, oracle, tm, nm, text, exact_strings=k % 2 == 0)
        assert doc.to_python() == json.loads(text.decode("utf-8"))


def _filler(tokens):
    """`tokens` tokens that leave an array expecting a value: '1,' pairs, an empty array in front for an odd count"""
    assert tokens >= 0 and tokens != 1
    if tokens % 2:
        return b"[]," + b"1," * ((tokens - 3) // 2)
    return b"1," * (tokens // 2)


FAR = BLOCK + 8   # tokens between a planted bracket and its partner on the far side
NEAR = 600        # ... and on the near side: the container crosses a border at most positions of the window
PLANTS = [
    ("number", lambda p: b"[" + _filler(p - 1) + b"-1.5e3,7]"),
    ("escaped_string", lambda p: b"[" + _filler(p - 1) + b'"a\\nb\\u20ac\\ud83d\\ude00",7]'),
    ("open_far_partner", lambda p: b"[" + _filler(p - 1) + b"[" + _filler(FAR) + b"1],7]"),
    ("close_near_partner", lambda p: b"[" + _filler(p - 1 - NEAR) + b"[" + _filler(NEAR - 2) + b"1],7]"),
]


@pytest.mark.parametrize("name,make", PLANTS, ids=[p[0] for p in PLANTS])
def test_block_borders(dev, oracle, tm, nm, name, make):
    """Each plant at every token position of a window of two blocks + 8 tokens around a block border."""
    items = []
    window = range(BLOCK - 4, 3 * BLOCK + 4)
    for p in window:
        data = make(p)
        a = arrays_of(oracle, nm, data)
        want_type = {"number": ord("-"), "escaped_string": ord('"'), "open_far_partner": ord("["), "close_near_partner": ord("]")}[name]
        assert a["typ"][p] == want_type, (name, p)
        if name == "open_far_partner":
            assert a["match"][p] == p + FAR + 2
        if name == "close_near_partner":
            assert a["match"][p] == p - NEAR
        items.append((data, a, {}))
    run_batch(dev, tm, items)


def _count_field(tape, pos):
    return (int(tape[pos]) >> 32) & 0xFFFFFF


def test_counts(dev, oracle, tm, nm):
    docs = {
        "siblings": b'[[1,2],[3,4,5],[],{"a":1,"b":[]}]',
        "flat": b"[" + b"1," * (3 * BLOCK) + b"1]",
        "object": b"{" + b",".join(b'"k%d":%d' % (k, k) for k in range(BLOCK)) + b"}",
        "objects": b"[" + b",".join(b'{"a":1,"b":[%d,2],"c":{}}' % k for k in range(600)) + b"]",
        # containers that open in one block and close two blocks later, at three levels at once
        "spanning": b'[1,[2,3,{"a":4,"b":[' + b"5," * (2 * BLOCK + 100) + b'6],"c":7,"d":8},9],10,11]',
        "deep": b"[" * 5000 + b"1,2" + b"]" * 5000,
    }
    items = [(d, arrays_of(oracle, nm, d), {}) for d in docs.values()]
    out = dict(zip(docs, run_batch(dev, tm, items)))
    # by hand, beside the twin
    t = out["siblings"][1]
    assert [_count_field(t, p) for p in (1, 2, 8, 16, 18, 23)] == [4, 2, 3, 0, 2, 0]
    assert _count_field(out["flat"][1], 1) == 3 * BLOCK + 1
    assert _count_field(out["object"][1], 1) == BLOCK
    t = out["spanning"][1]
    # r [ 1 1 [ 2 2 3 3 { "a" 4 4 "b" [: the four containers open at words 1, 4, 9 and 14
    assert [_count_field(t, p) for p in (1, 4, 9, 14)] == [4, 4, 4, 2 * BLOCK + 101]
    assert [int(t[p]) >> 56 for p in (1, 4, 9, 14)] == [ord(c) for c in "[[{["]
    t = out["deep"][1]
    assert [_count_field(t, p) for p in range(1, 5001)] == [1] * 4999 + [2]
    # and through the real chain, the deep one with max_depth raised accordingly
    check_chain(dev, oracle, tm, nm, docs["deep"], max_depth=6000)
    check_chain(dev, oracle, tm, nm, docs["spanning"])
    check_chain(dev, oracle, tm, nm, docs["flat"])


def _body(length, unit):
    """A body of exactly `length` bytes made of `unit` and 'x' padding"""
    k = length // len(unit) if unit else 0
    return unit * k + b"x" * (length - k * len(unit))


def _run_body(length):
    """... that is a single run of 2k backslashes (and one 'x' if the length is odd)"""
    run = length & ~1
    return b"\\" * run + b"x" * (length - run)


UNITS = [("plain", b""), ("n", b"\\nab"), ("bs_t", b"\\\\\\tq"), ("e9", b"\\u00e9z"), ("20ac", b"\\u20ac"), ("pair", b"\\ud83d\\ude00")]
UNIT_OUT = {"plain": 0, "n": 3, "bs_t": 3, "e9": 3, "20ac": 3, "pair": 4}  # unescaped bytes per unit


@pytest.mark.parametrize("length", [0, 1, LANE_BODY - 1, LANE_BODY, LANE_BODY + 1, 4097, 70000, (1 << 20) + 4097])
def test_strings(dev, oracle, tm, nm, length):
    """A key and a value of the same body, and a string behind them: ulen, the length prefixes, the bytes and the offsets,
    with and without the string buffer."""
    items, want_ulen = [], []
    for name, unit in UNITS + [("run", None)]:
        body = _run_body(length) if unit is None else _body(length, unit)
        if unit is None:
            ulen = (length & ~1) // 2 + (length & 1)
        elif unit:
            k = length // len(unit)
            ulen = k * UNIT_OUT[name] + (length - k * len(unit))
        else:
            ulen = length
        data = b'{"' + body + b'":"' + body + b'","after":["z","' + body[:len(body) & ~1] + b'"]}'
        items.append((data, arrays_of(oracle, nm, data), {}))
        want_ulen.append(ulen)
    out = run_batch(dev, tm, items)
    for (res, tape, sbuf), ulen, (name, _) in zip(out, want_ulen, UNITS + [("run", None)]):
        # the records by hand: key at 0, value behind it, then "after", "z" and the last body
        pre = lambda off: int(np.frombuffer(sbuf[off:off + 4].tobytes(), dtype="<u4")[0])
        assert pre(0) == ulen and pre(4 + ulen) == ulen, (name, length, pre(0), ulen)
        assert pre(8 + 2 * ulen) == 5 and sbuf[12 + 2 * ulen:17 + 2 * ulen].tobytes() == b"after"
        assert pre(17 + 2 * ulen) == 1 and sbuf[21 + 2 * ulen] == ord("z")
        offs = [int(tape[p]) & ((1 << 56) - 1) for p in (2, 3, 4, 6, 7)]
        assert offs == [0, 4 + ulen, 8 + 2 * ulen, 17 + 2 * ulen, 22 + 2 * ulen], (name, length, offs)
        assert sbuf[4:4 + ulen].tobytes() == sbuf[8 + ulen:8 + 2 * ulen].tobytes()
        assert res.n_strings == 5
    layout = run_batch(dev, tm, items, strings=False)
    for (res, tape, _), (res2, tape2, _) in zip(out, layout):
        assert res2.code == 0 and res2.string_bytes == res.string_bytes and np.array_equal(tape, tape2)


def test_capacities(dev, oracle, tm, nm):
    """One short of the tape, one short of the string buffer, fewer number records than numbers: MSJ_CAPACITY, the true
    sizes, nothing behind a capacity (run_batch's canaries)."""
    long_body = _body(5000, b"\\u20ac")
    docs = [b'{"k":["abc",1.5,"\\u20ac"],"z":-7}', b'["' + long_body + b'",1,2,"tail"]',
            b"[" + b'"s\\n",1.5,' * (BLOCK + 3) + b"null]"]
    for data in docs:
        a = arrays_of(oracle, nm, data)
        full, _, _ = ttm.twin_build(tm, data, a)
        nn = a["bits"].size
        items = [(data, a, {}), (data, a, {"tape_capacity": int(full.tape_words) - 1}), (data, a, {"string_capacity": int(full.string_bytes) - 1}),
                 (data, a, {"numbers_capacity": nn - 1}), (data, a, {"tape_capacity": 2, "string_capacity": 3, "numbers_capacity": 0}),
                 (data, a, {"tape_capacity": int(full.tape_words), "string_capacity": int(full.string_bytes)})]
        out = run_batch(dev, tm, items)
        sizes = (full.tape_words, full.string_bytes, full.n_strings)
        for j, (res, _, _) in enumerate(out):
            assert (res.tape_words, res.string_bytes, res.n_strings) == sizes
            assert res.code == (0 if j in (0, 5) else MSJ_CAPACITY), j
        # the layout-only form does not look at the string capacity
        res = run_batch(dev, tm, [(data, a, {"string_capacity": 0})], strings=False)[0][0]
        assert res.code == 0 and res.string_bytes == full.string_bytes


def test_verdict_not_zero_writes_only_the_result(dev, oracle, tm, nm):
    """d_verdict with a code: only d_result is written.  The same (invalid) arrays without a verdict: the call returns
    without writing past any capacity; the contents are not compared."""
    bad = [b'[1,2,"a\\qb",{"k":tru}]', b"[1,2", b'{"a":[1,2}]', b"]]],1,[[", b'["\\ud800",1e999,01]', b'{"a" "b" [ ] } , , ,',
           b"[" + b"1," * (2 * BLOCK) + b'"\\u12"', b'"' + b"\\" * 3000 + b'q"']
    items = []
    for data in bad:
        a = ttm.host_arrays(oracle, nm, data)
        if isinstance(a, int):
            continue
        items.append((data, a, {}))
    assert len(items) >= 6
    out = run_batch(dev, tm, items, verdict_code=tvm.TAPE)
    assert all(r.code == tvm.TAPE for r, _, _ in out)
    for caps in ({}, {"tape_capacity": 3, "string_capacity": 5, "numbers_capacity": 0}):
        run_batch(dev, tm, [(d, a, caps) for d, a, _ in items], compare=False)
    # a verdict of 0 changes nothing
    good = b'{"a":[1,"x\\n"]}'
    a = arrays_of(oracle, nm, good)
    r0 = run_batch(dev, tm, [(good, a, {})])[0]
    r1 = run_batch(dev, tm, [(good, a, {})], verdict_code=0)[0]
    assert r1[0].code == 0 and np.array_equal(r0[1], r1[1]) and np.array_equal(r0[2], r1[2])
    # the chain: an invalid document ends with the verdict's code in both results
    got = device_document(dev, b'[1,2,"a\\qb"]')
    assert got[0].code == tvm.STRING and (got[1].code, got[1].tape_words, got[1].string_bytes) == (tvm.STRING, 0, 0)
    assert device_document(dev, b'["abc') == 15  # MSJ_UNCLOSED_STRING


def test_bad_arguments_launch_nothing(dev):
    import torch

    data = b'[1,"a"]'
    d_buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev.device)
    d_idx = torch.empty(16, dtype=torch.int32, device=dev.device)
    d_carry = dev.new_carry()
    dev.index(d_buf, d_idx, d_carry)
    n = int(dev.fetch(d_carry).count)
    d_type, d_depth, _, d_match, d_end, d_flags = dev.stage2_prep(d_buf, len(data), d_idx, n, match=True)
    d_numbers, _ = dev.number_values(d_buf, len(data), d_idx, n, d_flags, capacity=4)
    d_verdict = torch.zeros(32, dtype=torch.uint8, device=dev.device)
    d_tape = torch.full((16,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev.device)
    d_sbuf = torch.full((64,), 0x5A, dtype=torch.uint8, device=dev.device)
    d_res = torch.full((32,), 0xAB, dtype=torch.uint8, device=dev.device)
    # by argument position
    tensors = {1: d_buf, 3: d_idx, 5: d_type, 6: d_depth, 7: d_match, 8: d_end, 9: d_flags, 10: d_numbers, 13: d_verdict, 14: d_tape,
               16: d_sbuf, 18: d_res}
    good = [dev.ctx, None, len(data), None, n, None, None, None, None, None, None, 4, None, None, None, 16, None, 64, None, dev._stream()]
    for k, t in tensors.items():
        good[k] = ctypes.c_void_p(t.data_ptr())

    def call(change=None):
        a = list(good)
        for k, v in (change or {}).items():
            a[k] = v
        return dev.lib.msj_tape_device(*a)

    assert call({4: 0}) == -1  # n == 0
    for k in (0, 1, 3, 5, 6, 7, 8, 9, 10, 14, 18):
        assert call({k: None}) == -1, k
    for k, off in ((3, 4), (6, 4), (7, 8), (8, 4), (10, 8), (14, 8), (5, 4), (9, 1), (13, 4), (18, 4)):  # off the 16-byte / 8-byte grid
        assert call({k: ctypes.c_void_p(tensors[k].data_ptr() + off)}) == -1, k
    assert call({12: ctypes.c_void_p(d_verdict.data_ptr() + 4)}) == -1
    assert call({2: 1 << 32}) == 1 and call({4: 1 << 31}) == 1  # MSJ_CAPACITY
    torch.cuda.synchronize()
    assert (d_res.cpu().numpy() == 0xAB).all() and (d_tape.cpu().numpy() == 0x5A5A5A5A5A5A5A5A).all()  # nothing was launched
    assert (d_sbuf.cpu().numpy() == 0x5A).all()
    assert call() == 0
    assert call({16: ctypes.c_void_p(d_sbuf.data_ptr() + 1), 17: 63}) == 0  # the string buffer needs no alignment
    assert call({16: None, 17: 0, 13: None, 10: None, 11: 0}) == 0  # layout only, no verdict, no number records
    torch.cuda.synchronize()
    res = d_res.cpu().numpy()
    assert res[:4].view(np.int32)[0] == MSJ_CAPACITY and res[8:16].view(np.uint64)[0] == 7  # r [ l 1 "a" ] r


def test_workspaces_grow_and_are_reused(oracle):
    """One context of its own through small, large, small, large: every workspace of the chain is allocated, outgrown and
    re-allocated, then reused twice (DeviceBuffer::reserve, csrc/ctx.h).  Each of the four results -- verdict, tape result,
    tape words, string bytes -- equals what a fresh context gives for the same document.  The large document is sized so
    that each workspace of the chain needs more than 1.25 times (the head-room factor) what the small one left."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd import _lib
    from mojo_simdjson_amd.device import Stage1Device

    # numbers, escaped strings and nesting in both; the large one is the small one's elements about 4 MiB long
    element = b'{"k":[1,-2.5e3,"' + _body(40, b"\\u20ac") + b'",{"x":[true,null,"a\\nb\\\\"]}],"z":[[],{}],"' + _body(30, b"\\tq") + b'":1e-7}'
    small = b"[" + element + b"," + element + b"," + PLANTS[1][1](8) + b"]"
    large = b"[" + (element + b",") * ((4 << 20) // (len(element) + 1)) + PLANTS[0][1](BLOCK + 5) + b"]"
    assert 200 <= len(small) <= 1000 and len(large) >= (4 << 20) - 1024

    lib = _lib.load()
    prep = lib.msj_stage2_prep_workspace_bytes
    prep.restype, prep.argtypes = ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]
    sizes = {}
    for name, data in (("small", small), ("large", large)):
        code, n, _ = helpers.run_oracle(oracle.msj_oracle_stage1, data)
        assert code == 0
        sizes[name] = (prep(n, len(data), 1), lib.msj_number_values_workspace_bytes(n, len(data)),
                       lib.msj_validate_workspace_bytes(n, len(data)), lib.msj_tape_workspace_bytes(n, len(data)))
    for s_bytes, l_bytes in zip(sizes["small"], sizes["large"]):
        assert 4 * l_bytes > 5 * s_bytes, (sizes["small"], sizes["large"])  # large > 1.25 x small: really re-allocated

    def run(d, data):
        got = device_document(d, data)
        assert not isinstance(got, int), got
        verdict, tres, d_tape, d_sbuf = got
        assert (verdict.code, tres.code) == (0, 0) and tres.tape_words > 2 and tres.string_bytes > 0
        return (bytes(verdict), bytes(tres), d_tape[:int(tres.tape_words)].cpu().numpy().tobytes(),
                d_sbuf[:int(tres.string_bytes)].cpu().numpy().tobytes())

    want = {}
    for name, data in (("small", small), ("large", large)):
        fresh = Stage1Device(0)
        want[name] = run(fresh, data)
        fresh.close()
    own = Stage1Device(0)
    try:
        for step, (name, data) in enumerate((("small", small), ("large", large), ("small", small), ("large", large))):
            got = run(own, data)
            for part, g, w in zip(("verdict", "tape result", "tape", "string buffer"), got, want[name]):
                assert g == w, (step, name, part)
    finally:
        own.close()


@pytest.mark.parametrize("workload", ["minified", "utf8", "pretty4"])
def test_workloads_1mib(dev, oracle, tm, nm, workload):
    from mojo_simdjson_amd import synth

    u = synth.workload(workload, 1 << 20).tobytes()
    doc = check_chain(dev, oracle, tm, nm, u)
    try:
        want = json.loads(u.decode("utf-8"))
    except (ValueError, UnicodeDecodeError):
        want = None  # (a workload json.loads does not take: the twin alone decides)
    if want is not None:
        assert doc.to_python() == want
    assert doc.tape.size > 1000 and doc.string_buf.size > 1000


def test_minified_1gib(dev, oracle, tm, nm):
    """1 GiB as ONE document ([unit,unit,...,last] of a 64 MiB unit and a small last element, as in
    tests/test_validate.py): the sizes, the root words and the root's count by hand; every repetition of the unit equal to the
    twin's tape of one unit up to the offsets of its position, compared on the device."""
    import torch

    from mojo_simdjson_amd import synth

    u = synth.workload("minified", 64 << 20)
    ub = u.tobytes()
    a = arrays_of(oracle, nm, ub)
    want, w_tape, w_sbuf = ttm.twin_build(tm, ub, a)
    wu, su = int(want.tape_words) - 2, int(want.string_bytes)  # words and string bytes of one unit
    unit = w_tape[1:1 + wu]
    tags = (unit >> np.uint64(56)).astype(np.int64)
    second = np.zeros(wu, dtype=bool)  # the value word of a number: not a tagged word
    k = 0
    while k < wu:
        if tags[k] in (ord("l"), ord("d")):
            second[k + 1] = True
            k += 2
        else:
            k += 1
    add_pos = (~second & np.isin(tags, [ord(c) for c in "{}[]"])).astype(np.int64)
    add_str = (~second & (tags == ord('"'))).astype(np.int64)
    reps = 16
    dv = dev.device
    d_unit = torch.from_numpy(u).to(dv)
    sep = torch.tensor([ord(",")], dtype=torch.uint8, device=dv)
    parts = [torch.tensor([ord("[")], dtype=torch.uint8, device=dv)]
    for r in range(reps):
        parts += [d_unit, sep] if r + 1 < reps else [d_unit]
    tail = b',{"end":true,"s":"a\\nb"}]'
    parts.append(torch.from_numpy(np.frombuffer(tail, dtype=np.uint8).copy()).to(dv))
    d_buf = torch.cat(parts)
    length = d_buf.numel()
    assert length > (1 << 30) - (1 << 20)
    del parts
    got = dev.parse_document(d_buf, length)
    assert not isinstance(got, int)
    verdict, tres, d_tape, d_sbuf = got
    assert (verdict.code, verdict.flags, tres.code, tres.flags) == (0, 0, 0, 0)
    E = 2 + reps * wu + 7  # root, '[', the units, { "end" true "s" "a\nb" } ]
    assert (tres.tape_words, tres.string_bytes, tres.n_strings) == (E + 1, reps * su + 19, reps * int(want.n_strings) + 3)
    head = d_tape[:2].cpu().numpy().view(np.uint64)
    assert int(head[0]) == (ord("r") << 56) | (E + 1)
    assert int(head[1]) == (ord("[") << 56) | ((reps + 1) << 32) | E
    last = d_tape[E - 8:E + 1].cpu().numpy().view(np.uint64)
    q = reps * su
    assert [int(x) for x in last[1:]] == [(ord("{") << 56) | (2 << 32) | (E - 1), (ord('"') << 56) | q, ord("t") << 56,
                                          (ord('"') << 56) | (q + 7), (ord('"') << 56) | (q + 12), (ord("}") << 56) | (E - 7),
                                          (ord("]") << 56) | 1, ord("r") << 56]
    assert d_sbuf[q:q + 19].cpu().numpy().tobytes() == b"\x03\0\0\0end\x01\0\0\0s\x03\0\0\0a\nb"
    d_want = torch.from_numpy(unit.view(np.int64)).to(dv)
    d_pos, d_str = torch.from_numpy(add_pos).to(dv), torch.from_numpy(add_str).to(dv)
    for r in range(reps):
        expect = d_want + d_pos * (1 + r * wu) + d_str * (r * su)
        have = d_tape[2 + r * wu:2 + (r + 1) * wu]
        diff = int((have != expect).sum())
        assert diff == 0, (r, diff)
    # the unit's string bytes: the first repetition equal to the twin's, the others equal to the first
    first = d_sbuf[:su]
    assert bool((first == torch.from_numpy(w_sbuf[:su]).to(dv)).all())
    for r in (1, reps // 2, reps - 1):
        assert bool((d_sbuf[r * su:(r + 1) * su] == first).all()), r
