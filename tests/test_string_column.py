"""A selected path's strings as one column on the device (msj_string_column_device, csrc/string_column_kernel.hip).

Expected values come from the host twin of the same arithmetic (tests/string_column_math_host.cpp), which
tests/test_string_column_math.py holds against the definition written in Python.  Device output is compared with the twin
over the WHOLE d_offsets, d_valid and d_bytes arrays (both start from the same fill, with 64 bytes of canary behind each
capacity, so a store the twin does not make shows).  Records come both ways: from the select twin, uploaded, and from the
real chain (shard, stage2_prep, documents, number_values, validate_documents, select_documents), whose device result the
call reads D from.  A block of sc_lengths / sc_copy is B = 256 rows.
"""

import numpy as np
import pytest

from tests import helpers
from tests import select_reference as ref
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

B = 256            # rows per workgroup of sc_lengths / sc_copy (csrc/string_column_kernel.hip: kRows)
LANE_BODY = tcm.LANE_BODY
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
        self.vtwin, self.stwin, self.ctwin = tdm.load_twin(), tsm.load_twin(), tcm.load_twin()
        self._paths = {}

    def paths(self, pointers):
        key = tuple(pointers)
        if key not in self._paths:
            self._paths[key] = self.dev.compile_paths(pointers)
        return self._paths[key]


def device_column(dev, d_buf, length, d_fields, p, d_sel, want):
    """msj_string_column_device with the twin's capacities, its arrays filled like the twin's with their canaries -> tcm.Column"""
    import torch

    offsets, valid, data = tcm.filled(want.capacity, want.bytes_capacity, want.data is None)
    d_off = torch.from_numpy(offsets.view(np.int64)).to(dev.device)
    d_valid = torch.from_numpy(valid).to(dev.device)
    d_bytes = torch.from_numpy(data).to(dev.device) if data is not None else None
    res, _, _, _ = dev.string_column(d_buf, length, d_fields, p, d_sel, d_offsets=d_off, d_valid=d_valid, d_bytes=d_bytes,
                                     capacity=want.capacity, bytes_capacity=want.bytes_capacity, strings=data is not None)
    return tcm.Column(res, d_off.cpu().numpy().view(np.uint64), d_valid.cpu().numpy(), d_bytes.cpu().numpy() if data is not None else None,
                      want.capacity, want.bytes_capacity)


def same(got, want, where=None):
    """The device's result and every array are the twin's, fill and canary included"""
    assert got.summary() == want.summary(), (where, got.summary(), want.summary())
    for name in ("offsets", "valid", "data"):
        a, b = getattr(got, name), getattr(want, name)
        if b is None:
            assert a is None
            continue
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (where, name, int(bad[0]), a[bad[:4]].tolist(), b[bad[:4]].tolist(), bad.size)


def upload_records(dev, records, code=0):
    """One path's records as d_fields of shape (1, rows, 2), and a select result that counts them"""
    rows = np.concatenate([np.ascontiguousarray(records), np.zeros(1, dtype=tsm.FIELD_DTYPE)])   # (never an empty tensor)
    d_fields = ttd.to_device(dev, rows).reshape(1, -1, 2)
    d_sel = ttd.to_device(dev, np.frombuffer(bytes(tcm.select_result(len(records), code)), dtype=np.uint8))
    return d_fields, d_sel


def check(env, lines, chain, pointer="/s", verdicts=False, where=None):
    """One window's column on the device against the twin, in the layout-only form and then with the bytes.  chain: the records
    and the select result of the real chain on the device, else the select twin's records uploaded; verdicts: the documents'
    verdicts are given to the select call.  -> (twin's Column, (code, value) per row)"""
    data = tdk.join(lines, b"\n")
    w = tdm.WindowArrays(env.oracle, env.nm, data, is_final=False)
    assert w.D == len(lines), where
    rows = tdm.twin_documents(env.vtwin, w, 100)[0] if verdicts else None
    got = tsm.twin_select(env.stwin, w, [pointer], verdicts=rows)
    values = tsm.check_against_reference(w, got, [pointer], lines, codes=[c for c, _ in rows] if rows else None)
    records = got.column(0)[:w.D].copy()
    if chain:
        a = tsd.FromChain(env.dev, data, False, verdicts)
        assert a.n == w.n, where
        d_sel, d_fields = env.dev.select_documents(env.paths([pointer]), a.d_buf, a.length, a.d_idx, a.n, a.d_type, a.d_depth, a.d_match,
                                                   a.d_end, a.d_flags, a.d_first, a.d_docs, d_numbers=a.d_numbers, numbers_capacity=a.ncap,
                                                   d_numbers_result=a.d_num, d_verdicts=a.d_verdicts, capacity=w.D + 3, sync=False)
        d_buf = a.d_buf
    else:
        d_buf = tvd.upload(env.dev, data)
        d_fields, d_sel = upload_records(env.dev, records)
    for layout_only in (True, False):
        want = tcm.twin_column(env.ctwin, data, records, w.D, layout_only=layout_only)
        same(device_column(env.dev, d_buf, len(data), d_fields, 0, d_sel, want), want, (where, layout_only))
        tcm.check_against_definition(want, [values[(0, k)] for k in range(w.D)], records)
    return want, [values[(0, k)] for k in range(w.D)]


def text(k, n):
    """A string of n characters that differs from row to row"""
    return "".join(chr(ord("a") + (k + j) % 26) for j in range(n))


def short_rows(n, start=0):
    return [text(k, k % 41) for k in range(start, start + n)]


@pytest.mark.parametrize("n", [1, B - 1, B, B + 1, 2 * B + 1])
def test_row_counts(env, n):
    """1 row, and B - 1, B, B + 1 and 2 B + 1 rows of lengths 0 .. 40: both ways in."""
    for chain in (False, True):
        want, _ = check(env, tcm.ndjson(short_rows(n)), chain, where=(n, chain))
        assert want.res.n_strings == n and want.res.total_bytes == sum(k % 41 for k in range(n))


def test_empty_rows(env):
    """2 B + 1 rows that are all "": no byte, and no byte of d_bytes touched.  Runs of 70 empty and non-string rows directly
    in front of and directly behind a block border, between short rows."""
    want, _ = check(env, tcm.ndjson([""] * (2 * B + 1)), chain=True)
    assert want.summary() == (0, 0, 2 * B + 1, 2 * B + 1, 0, 0, 0) and want.untouched(2 * B + 1, 0)
    for lo in (B - 70, B, 2 * B - 70, 0):
        values = short_rows(2 * B + 30)
        for k in range(lo, lo + 70):
            values[k] = ("", 7, None, "")[k % 4]
        want, _ = check(env, tcm.ndjson(values), chain=lo == B, where=lo)
        assert want.res.n_other == 35 and want.res.n_strings == 2 * B + 30 - 35


def test_long_plain_body(env):
    """One plain body of 70 000 bytes between short rows: the copy loop of its block makes hundreds of rounds."""
    values = short_rows(B + 40)
    values[B + 3] = text(5, 70000)
    for chain in (False, True):
        want, _ = check(env, tcm.ndjson(values), chain, where=chain)
    assert want.res.total_bytes > 70000 and want.rows()[B + 3] == text(5, 70000).encode()


def test_escaped_rows(env):
    """Escaped values on the first and the last row of a block; bodies of exactly kLaneBody raw bytes and of one more (the
    lane's walk and the wave's); a body of 70 002 raw bytes that is all \\u00e9 (a third of that in the output); two long
    bodies in one block."""
    values = short_rows(2 * B + 1)
    for k in (0, B - 1, B, 2 * B - 1, 2 * B):
        values[k] = "q\"%d\\\n\t€\U0001F600/" % k
    lines = tcm.ndjson(values)
    lines[B - 1] = b'{"s":"\\u0041\\ud83d\\ude00\\n\\u20ac\\/"}'
    lines[7] = tcm.ndjson(["a" * (LANE_BODY - 2) + "\n"])[0]
    lines[B + 9] = tcm.ndjson(["b" * (LANE_BODY - 1) + "\n"])[0]
    lines[B + 20] = b'{"s":"' + b"\\u00e9" * 11667 + b'"}'
    lines[B + 120] = tcm.ndjson(["\t" + "c" * 5000 + "\\"])[0]
    for chain in (False, True):
        want, _ = check(env, lines, chain, where=chain)
    rows = want.rows()
    assert [len(rows[k]) for k in (7, B + 9, B + 20, B + 120)] == [LANE_BODY - 1, LANE_BODY, 2 * 11667, 5002]
    assert rows[B - 1] == "A\U0001F600\n€/".encode() and want.res.n_escaped == 5 + 4


def test_mixed_column_with_an_invalid_document(env):
    """Strings, numbers, containers, atoms, missing keys and a document with a verdict code, cycling across a block border."""
    kinds = ["str", 12, {"a": 1}, [1, "x"], True, None, -2.5, "", b'{"t":"no s"}', b'{"s":"ok","bad":[tru]}', "esc\n"]
    values = [kinds[k % len(kinds)] for k in range(B + 60)]
    values = [text(k, 9) if v == "str" else v for k, v in enumerate(values)]
    for chain in (False, True):
        want, vals = check(env, tcm.ndjson(values), chain, verdicts=True, where=chain)
    codes = [c for c, _ in vals]
    assert codes[8] == ref.NO_SUCH_FIELD and codes[9] == tvm.T_ATOM and want.rows()[9] is None and want.rows()[10] == b"esc\n"
    assert want.res.n_other > 100 and want.res.n_strings > 50 and want.res.n_rows - want.res.n_strings - want.res.n_other > 40


def test_capacities(env):
    """bytes_capacity one short and 0: clipped, the rest complete.  D > capacity: nothing but the result.  A select call
    that ran out of capacity itself: its code, nothing written."""
    import torch

    dev = env.dev
    values = short_rows(B + 5)
    values[3], values[B] = "e\n" * 30, "f\\" * 700
    lines = tcm.ndjson(values)
    data = tdk.join(lines, b"\n")
    w = tdm.WindowArrays(env.oracle, env.nm, data, is_final=False)
    records = tsm.twin_select(env.stwin, w, ["/s"]).column(0)[:w.D].copy()
    d_buf = tvd.upload(dev, data)
    d_fields, d_sel = upload_records(dev, records)
    total = int(tcm.twin_column(env.ctwin, data, records, w.D, layout_only=True).res.total_bytes)
    for kw in (dict(bytes_capacity=total - 1), dict(bytes_capacity=0), dict(bytes_capacity=total // 2), dict(capacity=w.D - 1, bytes_capacity=total),
               dict(capacity=w.D + 300, bytes_capacity=total + 100)):
        want = tcm.twin_column(env.ctwin, data, records, w.D, **kw)
        same(device_column(dev, d_buf, len(data), d_fields, 0, d_sel, want), want, kw)
        if "capacity" not in kw:
            assert want.res.code == MSJ_CAPACITY and want.res.total_bytes == total and want.untouched(w.D, kw["bytes_capacity"])
    assert want.res.code == 0
    over = tcm.twin_column(env.ctwin, data, records, w.D, capacity=w.D - 1, bytes_capacity=total)
    assert over.summary() == (MSJ_CAPACITY, 0, w.D, 0, 0, 0, 0) and over.untouched(-1, 0)
    # the real select call with one record too few: its result has MSJ_CAPACITY, and so has the column's
    a = tsd.FromChain(dev, data, False, True)
    d_res, d_f = dev.select_documents(env.paths(["/s"]), a.d_buf, a.length, a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end, a.d_flags,
                                      a.d_first, a.d_docs, d_numbers=a.d_numbers, numbers_capacity=a.ncap, d_numbers_result=a.d_num,
                                      d_verdicts=a.d_verdicts, capacity=w.D - 1, sync=False)
    want = tcm.twin_column(env.ctwin, data, records, w.D, sel_code=MSJ_CAPACITY, bytes_capacity=total)
    got = device_column(dev, a.d_buf, len(data), d_f, 0, d_res, want)
    same(got, want)
    assert got.summary() == (MSJ_CAPACITY, 0, 0, 0, 0, 0, 0) and got.untouched(-1, 0)
    # no row at all: offsets[0] and a zero result
    d_fields0, d_sel0 = upload_records(dev, records[:0])
    want = tcm.twin_column(env.ctwin, data, records, 0, capacity=4, bytes_capacity=8)
    same(device_column(dev, d_buf, len(data), d_fields, 0, d_sel0, want), want)
    assert want.offsets[0] == 0 and want.summary() == (0,) * 7
    torch.cuda.synchronize()


def test_spans_past_the_window(env):
    """Hand-made records whose spans run past len, among good ones, across a block border.  The len passed is SMALLER than
    the uploaded buffer, so even a kernel that read them would stay inside the allocation: they come back not valid."""
    data = bytes(range(32, 127)) * 40
    length = len(data) - 1000
    recs = []
    for k in range(B + 40):
        if k % 5 == 0:
            recs.append(tcm.record(length - 10, 11 + k % 7))                 # ends 1 .. 7 bytes past len
        elif k % 5 == 1:
            recs.append(tcm.record(length + k, 3))                           # starts past len
        elif k % 5 == 2:
            recs.append(tcm.record(length - (k % 9), k % 9))                 # ends exactly at len
        elif k % 5 == 3:
            recs.append(tcm.record(0xFFFFFFFF, 0xFFFFFFFF, flags=2))         # the largest span a record can name
        else:
            recs.append(tcm.record(k, k % 30))
    records = np.concatenate(recs)
    d_buf = tvd.upload(env.dev, data)
    d_fields, d_sel = upload_records(env.dev, records)
    want = tcm.twin_column(env.ctwin, data, records, len(records), length=length)
    same(device_column(env.dev, d_buf, length, d_fields, 0, d_sel, want), want)
    rows = want.rows()
    assert all((rows[k] is None) == (k % 5 in (0, 1, 3)) for k in range(len(rows)))
    assert rows[2] == data[length - 2:length] and want.res.n_other == sum(k % 5 in (0, 1, 3) for k in range(len(rows)))


def test_bad_arguments(env):
    """Each is refused with nothing launched: the outputs keep what was in them."""
    import torch

    dev = env.dev
    data = tdk.join(tcm.ndjson(["a", "bc"]), b"\n")
    w = tdm.WindowArrays(env.oracle, env.nm, data, is_final=False)
    records = tsm.twin_select(env.stwin, w, ["/s"]).column(0)[:w.D].copy()
    d_buf = tvd.upload(dev, data)
    d_fields, d_sel = upload_records(dev, records)
    sent = torch.full((8,), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    off = torch.full((8,), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    val = torch.full((16,), 0x5A, dtype=torch.uint8, device=dev.device)
    out = torch.full((16,), 0x5A, dtype=torch.uint8, device=dev.device)

    def call(**kw):
        p = dict(buf=d_buf.data_ptr(), len=len(data), col=d_fields.data_ptr(), sel=d_sel.data_ptr(), off=off.data_ptr(), val=val.data_ptr(),
                 cap=2, out=out.data_ptr(), room=16, res=sent.data_ptr())
        p.update(kw)
        return dev.lib.msj_string_column_device(dev.ctx, p["buf"], p["len"], p["col"], p["sel"], p["off"], p["val"], p["cap"], p["out"],
                                                p["room"], p["res"], dev._stream())

    assert call(len=(1 << 32) + 16) == MSJ_CAPACITY
    for name in ("res", "sel", "buf", "col", "off", "val", "out"):
        assert call(**{name: None}) == BAD_ARGUMENT, name
    for name, base, step in (("col", d_fields, 8), ("off", off, 4), ("sel", d_sel, 4), ("res", sent, 4)):
        assert call(**{name: base.data_ptr() + step}) == BAD_ARGUMENT, name
    torch.cuda.synchronize()
    assert bool((sent == tvd.SENTINEL).all()) and bool((off == tvd.SENTINEL).all()) and bool((val == 0x5A).all()) and bool((out == 0x5A).all())
    assert dev.lib.msj_string_column_workspace_bytes(0) > 0
    # unaligned d_valid / d_bytes, the layout-only form, and no capacity at all with NULL arrays (D > 0: MSJ_CAPACITY in the result)
    assert call(val=val.data_ptr() + 1, out=out.data_ptr() + 3, room=3) == 0 and call(out=None, room=0) == 0
    assert call(col=None, off=None, val=None, cap=0, out=None, room=0) == 0
    torch.cuda.synchronize()
    assert sent.cpu().numpy()[:6].tolist() == [MSJ_CAPACITY, 2, 0, 0, 0, 0]
    assert out.cpu().numpy()[3:6].tobytes() == b"abc" and val.cpu().numpy()[1:3].tolist() == [1, 1] and off.cpu().numpy()[:3].tolist() == [0, 1, 3]


def test_document_stream_strings_and_numbers(env):
    """A few hundred lines of seeded NDJSON through windows of 4 096 bytes, DocumentStream(select=["/id", "/user/name"]):
    Window.strings sliced back on the host and Window.number_column for both dtypes equal the reference's value of every
    document; an injected bad line, a string id and a float id are in it.  Without select both raise."""
    import torch
    from mojo_simdjson_amd.document_stream import DocumentStream

    dev = env.dev
    lines = ttd.ndjson_lines(200 << 10)[:300]
    bad_at = len(lines) // 2
    lines[bad_at] = b'{"id":1,"a":[1,2,tru]}'
    lines[3] = b'{"id":"dup","id":2,"user":7}'
    lines[5] = b'{"id":-2.5,"user":{"name":"e\\u0301\\n\\ud83d\\ude00"}}'
    lines[6] = b'{"user":{"name":""}}'
    data = b"\n".join(lines) + b"\n"
    decoded = [None if k == bad_at else ref.decode(x) for k, x in enumerate(lines)]
    pointers = ["/id", "/user/name"]
    want = {p: [(tvm.T_ATOM, None) if d is None else ref.lookup(d, p) for d in decoded] for p in pointers}
    stream = DocumentStream(dev, tvd.upload(dev, data), len(data), window=4096, select=pointers)
    strings = {p: [] for p in pointers}
    ints, floats = [], []
    windows = 0
    for win in stream:
        for p in pointers:
            offsets, out, valid = win.strings(p, bytes_capacity=1 if windows % 2 else None)   # (1: the buffer has to grow)
            assert offsets.dtype == torch.int64 and out.dtype == torch.uint8 and valid.dtype == torch.bool and offsets.is_cuda and out.is_cuda
            assert offsets.shape == (win.n_documents + 1,) and valid.shape == (win.n_documents,)
            off, raw, ok = offsets.cpu().tolist(), out.cpu().numpy().tobytes(), valid.cpu().tolist()
            assert off[-1] == len(raw)
            strings[p] += [raw[off[k]:off[k + 1]].decode("utf-8") if ok[k] else None for k in range(win.n_documents)]
        assert win.strings(1)[1].equal(win.strings("/user/name")[1])
        for dtype, acc in ((torch.int64, ints), (torch.float64, floats)):
            values, valid = win.number_column("/id", dtype)
            assert values.dtype == dtype and valid.dtype == torch.bool and values.is_cuda and values.shape == valid.shape == (win.n_documents,)
            acc += [v if ok else None for v, ok in zip(values.cpu().tolist(), valid.cpu().tolist())]
        windows += 1
    assert windows >= 3 and len(ints) == len(lines)
    for p in pointers:
        assert strings[p] == [v if c == 0 and isinstance(v, str) else None for c, v in want[p]], p
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)
    assert ints == [v if c == 0 and is_int(v) else None for c, v in want["/id"]]
    assert floats == [float(v) if c == 0 and (is_int(v) or isinstance(v, float)) else None for c, v in want["/id"]]
    assert strings["/id"][3] == "dup" and floats[5] == -2.5 and ints[5] is None and strings["/user/name"][5] == "é\n\U0001F600"
    assert strings["/user/name"][6] == "" and sum(v is not None for v in strings["/user/name"]) > 250 and sum(v is not None for v in ints) > 250
    plain = next(iter(DocumentStream(dev, tvd.upload(dev, data), len(data), window=4096, validate=True)))
    for call in (plain.strings, plain.number_column):
        with pytest.raises(ValueError):
            call(0)
