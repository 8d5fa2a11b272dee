"""Timestamps and numbers written as strings on the device (msj_cast_strings_device, csrc/cast_strings_kernel.hip).

Expected values come from the host twin of the same arithmetic (tests/cast_strings_math_host.cpp), which
tests/test_cast_strings_math.py holds against a yardstick written in Python.  Device output is compared with the twin over the
WHOLE record array (both start from the same fill, with 64 bytes of canary behind the capacity, so a store the twin does not
make shows) and over the result and the select result.  Records are generated on the host and uploaded; the end-to-end test
runs the real chain through DocumentStream.  Every comparison runs with both forms of the kernel's byte fetch
(msj_debug_set_cast_fetch), which have to write the same records.

The kernel's constants (csrc/cast_strings_kernel.hip) are named below as the shapes use them.
"""
import ctypes
import datetime
import json
import random

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from mojo_simdjson_amd.document_stream import FIELD_DTYPE
from tests import test_cast_strings_math as tcs
from tests import test_string_column_math as tcm
from tests import test_tape_documents as ttd
from tests import test_validate_documents as tvd

pytestmark = pytest.mark.gpu

B = 256                  # kRows: rows per workgroup, one per lane
ROW_GRID = 4096 * B      # kGridBlocks = 4096 blocks of kRows rows, `v += gridDim.x`
WAVE = 64
BEHIND = 0x37            # the bytes behind the window's length on the device: '7', a digit
MSJ_CAPACITY, BAD_ARGUMENT = 1, -1
TIMESTAMP, NUMBER, KEEP = tcs.TIMESTAMP, tcs.NUMBER, tcs.KEEP_NUMBERS
FETCHES = (_lib.CAST_FETCH_WINDOW, _lib.CAST_FETCH_BYTES)

TS35 = b"2024-05-01T12:34:56.123456789+05:30"
TS20 = b"2024-05-01T12:34:56Z"
NUM17 = b"90071992547409931"


@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    d = Stage1Device(0)
    yield d
    d.lib.msj_debug_set_cast_fetch(d.ctx, _lib.CAST_FETCH_WINDOW)
    d.close()


@pytest.fixture(scope="module")
def ctw():
    return tcs.load_twin()


def struct_to_device(dev, s):
    import torch

    return torch.from_numpy(np.frombuffer(bytes(s), dtype=np.uint8).copy()).to(dev.device)


def upload_window(dev, data, length=None):
    """The first `length` bytes of data, BEHIND from there on: what the device may not let change a verdict"""
    length = len(data) if length is None else length
    return tvd.upload(dev, data[:length] + bytes([BEHIND]) * 64)


def run_cast(dev, ctw, data, records, kind, unit="s", flags=0, R=None, capacity=None, sel_code=0, in_place=False, length=None, where=None,
             fetches=FETCHES):
    """The device, with each form of the fetch, against the twin over the whole of the record array -> the twin's tcs.Cast"""
    import torch

    records = np.ascontiguousarray(records)
    R = len(records) if R is None else R
    capacity = len(records) if capacity is None else capacity
    length = len(data) if length is None else length
    want = tcs.twin_cast(ctw, data[:length], records, kind, unit, flags, R=R, length=length, capacity=capacity, sel_code=sel_code, in_place=in_place)
    assert want.rc == 0
    d_buf = upload_window(dev, data, length)
    d_rows = ttd.to_device(dev, np.concatenate([records, np.zeros(1, dtype=FIELD_DTYPE)]))
    t_sel = struct_to_device(dev, tcm.select_result(R, sel_code))
    for fetch in fetches:
        assert dev.lib.msj_debug_set_cast_fetch(dev.ctx, fetch) == 0
        start = np.full(16 * capacity + tcs.CANARY, tcs.FILL, dtype=np.uint8)
        if in_place:
            start[:16 * len(records)] = records.view(np.uint8)
        t_out = torch.from_numpy(start).to(dev.device)
        t_res = torch.full((48,), tcs.FILL, dtype=torch.uint8, device=dev.device)
        t_osel = torch.full((48,), tcs.FILL, dtype=torch.uint8, device=dev.device)
        rc = dev.lib.msj_cast_strings_device(dev.ctx, d_buf.data_ptr(), length, t_out.data_ptr() if in_place else d_rows.data_ptr(), t_sel.data_ptr(),
                                             kind, tcs.UNITS[unit], flags, t_out.data_ptr(), capacity, t_res.data_ptr(), t_osel.data_ptr(),
                                             dev._stream())
        assert rc == 0, (where, fetch, rc)
        torch.cuda.synchronize()
        res = _lib.MsjCastStringsResult.from_buffer_copy(t_res.cpu().numpy().tobytes())
        osel = _lib.MsjSelectDocumentsResult.from_buffer_copy(t_osel.cpu().numpy().tobytes())
        got = tcs.Cast(rc, res, osel, t_out.cpu().numpy(), capacity)
        assert got.summary() == want.summary(), (where, fetch, got.summary(), want.summary())
        bad = np.nonzero(got.out != want.out)[0]
        if bad.size:
            k = int(bad[0]) // 16
            raise AssertionError((where, fetch, "record", k, tcs.as_tuple(records[k]) if k < len(records) else None,
                                  got.out[16 * k:16 * k + 16].tolist(), want.out[16 * k:16 * k + 16].tolist(), int(bad.size)))
    return want


def corpus(kind):
    return tcs.mixed_corpus(kind)


def cycle(records, n):
    return np.resize(records, n) if n else records[:0]


# ---- row counts ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [TIMESTAMP, NUMBER])
@pytest.mark.parametrize("n", [0, 1, B - 1, B, B + 1])
def test_row_counts(dev, ctw, kind, n):
    data, records = corpus(kind)
    for flags in (0, KEEP):
        want = run_cast(dev, ctw, data, cycle(records, n), kind, "ns" if kind == TIMESTAMP else "s", flags, where=n)
        assert want.res.n_rows == n and (n < B or want.res.n_cast > 0)


@pytest.mark.parametrize("kind", [TIMESTAMP, NUMBER])
def test_past_the_row_grid(dev, ctw, kind):
    """The grid's second trip: block 4096 is block 0's workgroup again"""
    data, records = corpus(kind)
    n = ROW_GRID + 1
    rows = cycle(records, n)
    rows[-1] = records[np.nonzero((records["type"] == ord('"')) & (records["flags"] == tcs.ESCAPED))[0][0]]   # the last row through the list
    want = run_cast(dev, ctw, data, rows, kind, "ms" if kind == TIMESTAMP else "s", KEEP, where="row grid", fetches=FETCHES[:1])
    assert want.res.n_rows == n and want.res.n_syntax > n // 20 and want.res.n_cast > n // 20


# ---- where the body lies ------------------------------------------------------------------------------------------------------

def test_body_phase(dev, ctw):
    """An accepted 35-byte timestamp, a 20-byte one and a 17-digit number, the body starting at every window offset mod 16"""
    data, recs = bytearray(), []
    for body in (TS35, TS20, NUM17):
        for phase in range(16):
            data += b'"' * (1 + (phase - len(data) - 1) % 16)
            assert len(data) % 16 == phase
            recs.append(tcs.rec(len(data) | (len(body) << 32), '"', token=len(recs)))
            data += body + b'"'
    records = np.concatenate(recs)
    for unit in tcs.UNITS:
        want = run_cast(dev, ctw, bytes(data), records, TIMESTAMP, unit, where=("phase", unit))
        assert want.res.n_cast == 32 and want.res.n_syntax == 16
    want = run_cast(dev, ctw, bytes(data), records, NUMBER, where="phase")
    assert want.res.n_cast == 16 and want.res.n_syntax == 32


@pytest.mark.parametrize("tail", range(16))
def test_window_ends(dev, ctw, tail):
    """The body as the very first and the very last bytes of the window, len % 16 = tail, digits behind len: a read past len
    would lengthen the fraction, the offset or the number"""
    for first, last, kind in ((TS35, b"2024-05-01T12:34:56.12", TIMESTAMP), (TS20[:-1], b"2024-05-01T12:34:56+05", TIMESTAMP),
                              (b"2024-05-01", b"2024-05-01T12:3", TIMESTAMP), (NUM17, b"1.5e1", NUMBER), (b"12", b"9", NUMBER)):
        fill = b'"' * ((tail - len(first) - len(last)) % 16 + 16)
        data = first + fill + last
        assert len(data) % 16 == tail
        records = np.concatenate([tcs.rec(0 | (len(first) << 32), '"', token=1), tcs.rec((len(data) - len(last)) | (len(last) << 32), '"', token=2),
                                  tcs.rec((len(data) - len(last)) | ((len(last) + 1) << 32), '"', token=3)])   # (one byte past: no string)
        want = run_cast(dev, ctw, data, records, kind, "ns" if kind == TIMESTAMP else "s", where=(tail, first))
        assert want.res.n_other == 1 and want.res.n_cast + want.res.n_syntax == 2 and want.res.n_cast >= 1
        # the same window cut in the middle of the last body: both records leave it
        run_cast(dev, ctw, data, records, kind, "ns" if kind == TIMESTAMP else "s", length=len(data) - 1, where=(tail, "cut"))


# ---- escaped rows: the list ---------------------------------------------------------------------------------------------------

def escaped_column(n, which, kind):
    """n string rows, those k with which(k) spelled with an escape"""
    values = [(b"2024-05-%02dT12:34:%02d.%03dZ" % (1 + k % 28, k % 60, k % 1000)) if kind == TIMESTAMP else b"%d.%02de-3" % (k * 7919, k % 100)
              for k in range(n)]
    bodies = [tcs.escape_at(v, k % len(v)) if which(k) else v for k, v in enumerate(values)]
    return tcs.window_of(bodies)


@pytest.mark.parametrize("kind", [TIMESTAMP, NUMBER])
@pytest.mark.parametrize("name", ["across a block border", "a block all escaped", "the last lane of a wave", "none", "one", "all"])
def test_escaped_rows(dev, ctw, kind, name):
    n, which = {"across a block border": (2 * B, lambda k: B - 5 <= k < B + 7), "a block all escaped": (3 * B - 1, lambda k: B <= k < 2 * B),
                "the last lane of a wave": (B + 1, lambda k: k == WAVE - 1), "none": (B + 3, lambda k: False), "one": (B + 3, lambda k: k == B + 2),
                "all": (2 * B + 1, lambda k: True)}[name]
    data, records = escaped_column(n, which, kind)
    assert int((records["flags"] == tcs.ESCAPED).sum()) == sum(1 for k in range(n) if which(k))
    want = run_cast(dev, ctw, data, records, kind, "us" if kind == TIMESTAMP else "s", where=name)
    assert want.res.n_cast == n


def test_numbers_that_need_the_exact_path(dev, ctw):
    """Numbers the fast paths cannot decide go through the list too, next to escaped ones"""
    rng = random.Random(8)
    texts = [t for t in tcs.tnm.fallback_texts(rng, 100) if len(t) <= 128]
    bodies = [tcs.escape_at(t, 0) if k % 5 == 0 else t for k, t in enumerate(texts)] + [b"1.5", b"7"] * 30
    rng.shuffle(bodies)
    data, records = tcs.window_of(bodies)
    want = run_cast(dev, ctw, data, records, NUMBER, where="exact")
    assert want.res.n_cast == len(bodies) > B


# ---- the corpus as one column -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, KEEP])
@pytest.mark.parametrize("kind,unit", [(TIMESTAMP, "s"), (TIMESTAMP, "ms"), (TIMESTAMP, "us"), (TIMESTAMP, "ns"), (NUMBER, "s")])
def test_corpus_as_one_column(dev, ctw, kind, unit, flags):
    data, records = corpus(kind)
    records = cycle(records, max(len(records), 2 * B + 37))
    want = run_cast(dev, ctw, data, records, kind, unit, flags, where=(kind, unit, flags))
    r = want.res
    assert len(records) > 2 * B and min(r.n_cast, r.n_syntax, r.n_other) > 0 and (unit not in ("ns", "s") or kind == TIMESTAMP and unit == "s" or r.n_range > 0)
    run_cast(dev, ctw, data, records, kind, unit, flags, in_place=True, where=(kind, unit, flags, "in place"))


def test_capacity_and_codes(dev, ctw):
    data, records = corpus(TIMESTAMP)
    n = len(records)
    want = run_cast(dev, ctw, data, records, TIMESTAMP, "ms", KEEP, capacity=n - 1, where="one short")
    assert want.res.code == MSJ_CAPACITY and want.res.n_rows == n and want.untouched(0)
    want = run_cast(dev, ctw, data, records, TIMESTAMP, "ms", sel_code=5, where="a code")
    assert want.res.code == 5 and want.sel.code == 5 and want.untouched(0)
    want = run_cast(dev, ctw, data, records, TIMESTAMP, "ms", R=n - 3, capacity=n + 5, where="room")
    assert want.res.code == 0 and want.untouched(n - 3)
    want = run_cast(dev, ctw, data, records[:4], TIMESTAMP, "ms", R=1 << 31, where="2^31")
    assert want.res.code == MSJ_CAPACITY and want.res.n_rows == 1 << 31


def hostile_records(rng, n, length):
    tags = [ord(c) for c in '""""ld{[tfn'] + [0, ord("x"), 0xFF]
    codes = [0, 0, 0, 0, 0, 0, 9, 17, 20, 3, 0xFFFF]
    out = np.zeros(n, dtype=FIELD_DTYPE)
    for k in range(n):
        b = rng.choice([length - 1, length, length + 1, 0xFFFFFFFF, 0, rng.randrange(length + 2), rng.randrange(length + 2)]) & 0xFFFFFFFF
        r = rng.choice([0, 1, 2, 10, 35, 36, 128, 129, 0xFFFFFFFF, rng.randrange(40), rng.randrange(300), 210, 211, 769])
        out[k] = (b | (r << 32) if rng.randrange(4) else rng.getrandbits(64), rng.getrandbits(32), rng.choice(tags),
                  (rng.getrandbits(8) & 2) if rng.randrange(4) else rng.getrandbits(8), rng.choice(codes))
    return out


@pytest.mark.parametrize("kind", [TIMESTAMP, NUMBER])
def test_hostile_records(dev, ctw, kind):
    """Spans at len - 1, len, len + 1 and 2^32 - 1, wild tags, flags and codes over a window of the grammar's bytes: no fault, the
    canaries intact, equal to the twin"""
    rng = random.Random(4242 + kind)
    alphabet = b'0123456789-:.TZ+ \\u00eE"'
    data = bytes(rng.choice(alphabet) if rng.randrange(8) else rng.getrandbits(8) for _ in range(3000)) + b"2024-05-01T12:34:56.789Z"
    records = hostile_records(rng, 3 * B + 17, len(data))
    for flags in (0, KEEP):
        want = run_cast(dev, ctw, data, records, kind, "ns" if kind == TIMESTAMP else "s", flags, where=("hostile", flags))
        assert want.res.n_syntax > 0 and want.res.n_other > 0
    run_cast(dev, ctw, data, records, kind, "s", KEEP, in_place=True, where="hostile in place")


# ---- the order of the argument checks -----------------------------------------------------------------------------------------

def test_check_order(dev):
    """Each is refused with nothing launched, in the header's order: the outputs keep what was in them"""
    import torch

    R = 8
    data, records = tcs.window_of([b"2024-05-0%d" % (k + 1) for k in range(R)])
    d_buf = upload_window(dev, data)
    d_rows = ttd.to_device(dev, np.concatenate([records, np.zeros(8, dtype=FIELD_DTYPE)]))
    sel = struct_to_device(dev, tcm.select_result(R))
    full = lambda n: torch.full((n,), 0x5A, dtype=torch.uint8, device=dev.device)
    out, res, osel = full(16 * (R + 4)), full(48), full(48)

    def cast(**kw):
        p = dict(ctx=dev.ctx, buf=d_buf.data_ptr(), len=len(data), rows=d_rows.data_ptr(), sel=sel.data_ptr(), kind=TIMESTAMP, unit=0, flags=0,
                 out=out.data_ptr(), cap=R, res=res.data_ptr(), osel=osel.data_ptr())
        p.update(kw)
        return dev.lib.msj_cast_strings_device(p["ctx"], p["buf"], p["len"], p["rows"], p["sel"], p["kind"], p["unit"], p["flags"], p["out"],
                                               p["cap"], p["res"], p["osel"], dev._stream())

    for name in ("ctx", "res", "sel", "buf", "rows", "out"):
        assert cast(**{name: None}) == BAD_ARGUMENT, name
    for bad in (dict(kind=0), dict(kind=3), dict(unit=4), dict(kind=NUMBER, unit=1), dict(flags=2), dict(kind=NUMBER, flags=4)):
        assert cast(**bad) == BAD_ARGUMENT, bad
    # NULL and the kind win over the size, the size over overlap, aliasing and alignment
    assert cast(len=(1 << 32) + 1, out=None) == BAD_ARGUMENT and cast(len=(1 << 32) + 1, kind=9) == BAD_ARGUMENT
    assert cast(len=(1 << 32) + 1, rows=d_rows.data_ptr() + 8) == MSJ_CAPACITY and cast(cap=1 << 40, res=sel.data_ptr()) == MSJ_CAPACITY
    assert cast(out=d_rows.data_ptr() + 16) == BAD_ARGUMENT and cast(out=d_rows.data_ptr() + 16 * (R - 1)) == BAD_ARGUMENT
    assert cast(rows=out.data_ptr() + 16 * (R - 1)) == BAD_ARGUMENT
    assert cast(res=sel.data_ptr()) == BAD_ARGUMENT and cast(osel=sel.data_ptr()) == BAD_ARGUMENT and cast(osel=res.data_ptr()) == BAD_ARGUMENT
    for name, base, step in (("rows", d_rows, 8), ("out", out, 8), ("sel", sel, 4), ("res", res, 4), ("osel", osel, 4)):
        assert cast(**{name: base.data_ptr() + step}) == BAD_ARGUMENT, name
    assert cast(cap=0, rows=None, out=None) == 0    # no room: the count alone is MSJ_CAPACITY
    torch.cuda.synchronize()
    assert _lib.MsjCastStringsResult.from_buffer_copy(res.cpu().numpy().tobytes()).code == MSJ_CAPACITY
    assert bool((out == 0x5A).all())
    res.fill_(0x5A), osel.fill_(0x5A)
    assert cast(osel=None) == 0
    torch.cuda.synchronize()
    assert bool((osel == 0x5A).all()) and bool((out[16 * R:] == 0x5A).all())
    got = out.cpu().numpy()[:16 * R].view(FIELD_DTYPE)
    assert got["bits"].tolist() == [1714521600 + 86400 * k for k in range(R)] and got["token"].tolist() == records["token"].tolist()
    assert got["type"].tolist() == [ord("l")] * R and got["code"].tolist() == [0] * R
    assert dev.lib.msj_debug_set_cast_fetch(dev.ctx, 2) == BAD_ARGUMENT and dev.lib.msj_debug_set_cast_fetch(None, 0) == BAD_ARGUMENT
    ws = dev.lib.msj_cast_strings_workspace_bytes
    assert ws(0) >= 64 and ws(1 << 20) >= ws(0) + 4 * (1 << 20) and ws(1 << 40) == ws(1 << 31)


# ---- end to end -------------------------------------------------------------------------------------------------------------

def ts_text(k):
    """Line k's timestamp: instants 250 ms apart from 2024-05-01T11:58:00Z, written with every offset, fraction width and
    separator in turn, so that neighbours differ in everything but order"""
    ms = 1714564680000 + 250 * k
    oh, om = [(0, 0), (5, 30), (-8, 0), (0, 0), (13, 45), (-3, -30)][k % 6]
    local = ms + (oh * 3600 + om * 60) * 1000
    days, rem = divmod(local, 86400000)
    date = datetime.date.fromordinal(days + 719163)
    text = "%04d-%02d-%02d%s%02d:%02d:%02d" % (date.year, date.month, date.day, "Tt "[k % 3], rem // 3600000, rem // 60000 % 60, rem // 1000 % 60)
    frac = "%03d" % (rem % 1000)
    text += ["." + frac, "," + frac + "000", "." + frac + "999999", "." + frac.rstrip("0") if frac.rstrip("0") else ""][k % 4]
    if (oh, om) == (0, 0):
        text += ["Z", "z", "+00:00", ""][k % 4]
    else:
        text += ("-" if oh < 0 else "+") + "%02d" % abs(oh) + [":", ""][k % 2] + "%02d" % abs(om)
    return text, ms


PRICES = ["12.50", "9007199254740993", "1e-3", "-0", "0.1", "1e400", "12,5", "", " 1", 12.5, 7, None, "3"]


def log_lines(n):
    lines, docs = [], []
    for k in range(n):
        text, ms = ts_text(k)
        d = {"ts": text, "price": PRICES[k % len(PRICES)], "stamps": [ts_text(k + 3 * j)[0] for j in range(k % 3)], "items": [{"at": ts_text(k + j)[0], "price": PRICES[(k + j) % len(PRICES)]} for j in range(k % 4)]}
        if k % 17 == 3:
            d["ts"] = ["not a time", 1714564680, None, "2024-02-30T00:00:00Z"][k // 17 % 4]
        if k % 19 == 4:
            del d["ts"]
        if d["price"] is None:
            del d["price"]
        line = json.dumps(d, indent=None if k % 2 else 1).encode()
        if k % 23 == 5 and isinstance(d.get("ts"), str):   # the same value spelled with an escape
            line = line.replace(b'"ts": "2', b'"ts": "\\u0032', 1)
        if k == 47:
            line, d = b'{"ts":"2024-05-01T12:00:00Z","items":[tru]}', None
        lines.append(line), docs.append(d)
    return lines, docs


def py_ms(v, unit="ms"):
    """The yardstick on a json.loads value: the int, or None"""
    if not isinstance(v, str):
        return None
    o, bits = tcs.py_timestamp(v.encode(), unit)
    return (bits - (1 << 64) if bits >> 63 else bits) if o == tcs.CAST else None


def py_num(v, keep=True):
    if isinstance(v, str):
        o, bits, tag = tcs.py_number(v.encode())
        if o != tcs.CAST:
            return None
        return float(int(bits - (1 << 64) if bits >> 63 else bits)) if tag == "l" else tcs.tnm.struct.unpack("<d", tcs.tnm.struct.pack("<Q", bits))[0]
    return float(v) if keep and isinstance(v, (int, float)) and not isinstance(v, bool) else None


def test_document_stream_casts(dev):
    """DocumentStream(select=["/ts", "/price", "/items", "/stamps"]) over 600 generated lines in several windows: timestamps, parsed_numbers
    and where(..., cast=...) against json.loads plus the Python yardstick; lines whose ts differ only in offset or fraction
    width sort the right way; the same over /items[*].at and /items[*].price; where without cast is what it was."""
    import torch
    from mojo_simdjson_amd.document_stream import DocumentStream, datetime_units

    lines, docs = log_lines(600)
    data = b"\n".join(lines) + b"\n"
    utc = datetime.timezone.utc
    dt0 = datetime.datetime(2024, 5, 1, 12, 0, 0, tzinfo=utc)
    dt1 = datetime.datetime(2024, 5, 1, 17, 31, 0, tzinfo=datetime.timezone(datetime.timedelta(hours=5, minutes=30)))   # 12:01:00Z
    t0, t1 = 1714564800000, 1714564860000
    assert datetime_units(dt0, "ms") == t0 and datetime_units(dt1, "ms") == t1 and datetime_units(dt0.replace(tzinfo=None), "ns") == t0 * 10**6
    assert datetime_units(datetime.datetime(1969, 12, 31, 23, 59, 59, 999999), "ms") == -1 and datetime_units(dt0, "s") == t0 // 1000
    seen = windows = kept_in_all = 0
    for win in DocumentStream(dev, tvd.upload(dev, data), len(data), window=32768, select=["/ts", "/price", "/items", "/stamps"]):
        D = win.n_documents
        mine = docs[seen:seen + D]
        want_ms = [py_ms(d.get("ts")) if d is not None else None for d in mine]
        for unit in ("s", "ms", "us", "ns"):
            values, valid = win.timestamps("/ts", unit)
            want = [py_ms(d.get("ts"), unit) if d is not None else None for d in mine]
            assert values.is_cuda and values.dtype == torch.int64 and valid.cpu().tolist() == [w is not None for w in want], (windows, unit)
            assert values.cpu().tolist() == [w or 0 for w in want], (windows, unit)
        order = [k for k in range(D) if want_ms[k] is not None]
        values = win.timestamps("/ts", "ms")[0].cpu().tolist()
        assert [values[k] for k in order] == sorted(values[k] for k in order) and len(set(values[k] for k in order)) == len(order)
        for keep in (True, False):
            values, valid = win.parsed_numbers("/price", keep_numbers=keep)
            want = [py_num(d.get("price"), keep) if d is not None else None for d in mine]
            assert valid.cpu().tolist() == [w is not None for w in want] and values.cpu().tolist() == [w or 0.0 for w in want], (windows, keep)
        ints, int_valid = win.parsed_numbers("/price", dtype=torch.int64)
        assert 9007199254740993 in ints.cpu().tolist() or D < len(PRICES)
        records, d_sel = win.cast("/ts", "timestamp", "ms")
        assert records.shape == (D, 2) and _lib.MsjSelectDocumentsResult.from_buffer_copy(d_sel.cpu().numpy().tobytes()).n_found == len(order)
        # the range as two exact int64 compares; the selection carries the original records
        sel = win.where([("/ts", ">=", dt0), ("/ts", "<", dt1)], cast={"/ts": ("timestamp", "ms")})
        want_rows = [k for k in range(D) if want_ms[k] is not None and t0 <= want_ms[k] < t1]
        assert sel.rows.cpu().tolist() == want_rows, windows
        assert sel.values("/ts") == [mine[k]["ts"] for k in want_rows] and sel.timestamps("/ts", "ms")[0].cpu().tolist() == [want_ms[k] for k in want_rows]
        same = win.where([("/ts", ">=", t0), ("/ts", "<", t1)], cast={"/ts": ("timestamp", "ms")})
        assert same.rows.cpu().tolist() == want_rows
        cheap = win.where([("/price", "<", 1), ("/ts", "<", dt1)], cast={"/price": "number", "/ts": "timestamp"})
        nums = [py_num(d.get("price")) if d is not None else None for d in mine]
        assert cheap.rows.cpu().tolist() == [k for k in range(D) if nums[k] is not None and nums[k] < 1 and want_ms[k] is not None and want_ms[k] < t1]
        with pytest.raises(ValueError):
            win.where([("/ts", ">=", dt0)])
        # without cast: a string is no number, as before
        assert win.where([("/ts", ">=", 1714564680)]).rows.cpu().tolist() == [k for k in range(D) if mine[k] is not None and
                                                                              isinstance(mine[k].get("ts"), int)]
        assert win.where([("/price", ">", 1)]).rows.cpu().tolist() == [k for k in range(D) if mine[k] is not None and
                                                                        isinstance(mine[k].get("price"), (int, float)) and mine[k]["price"] > 1]
        # the timestamps inside a list
        items = win.elements("/items")
        flat = [x for d in mine if d is not None and isinstance(d.get("items"), list) for x in d["items"]]
        fields = items.select(["/at", "/price"])
        values, valid = fields.timestamps("/at", "ms")
        assert valid.cpu().tolist() == [True] * len(flat) and values.cpu().tolist() == [py_ms(x["at"]) for x in flat]
        values, valid = fields.parsed_numbers("/price")
        assert valid.cpu().tolist() == [py_num(x.get("price")) is not None for x in flat]
        assert values.cpu().tolist() == [py_num(x.get("price")) or 0.0 for x in flat]
        late = fields.where([("/at", ">=", dt0)], cast={"/at": ("timestamp", "ms")})
        assert late.values("/at") == [x["at"] for x in flat if py_ms(x["at"]) >= t0]
        # a list of timestamps: the elements themselves are column 0
        stamps = win.elements("/stamps")
        flat = [x for d in mine if d is not None for x in d["stamps"]]
        values, valid = stamps.timestamps("us")
        assert valid.cpu().tolist() == [True] * len(flat) and values.cpu().tolist() == [py_ms(x, "us") for x in flat]
        early = stamps.where([(0, "<", dt0)], cast={0: ("timestamp", "s")})
        assert early.to_python() == [[x for x in d["stamps"] if py_ms(x) < t0] if d is not None else None for d in mine]
        seen += D
        windows += 1
        kept_in_all += len(want_rows)
    assert windows >= 3 and seen == len(docs) and kept_in_all >= 100
