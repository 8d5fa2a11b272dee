"""Numbers floored to buckets and byte keys from several columns on the device (msj_bucket_rows_device and
msj_group_keys_device, csrc/group_keys_kernel.hip), through the C ABI.

Expected values come from the host twin of the same arithmetic (tests/group_keys_math_host.cpp), which
tests/test_group_keys_math.py holds against the definition written in Python.  Device output is compared over WHOLE tensors:
every array starts from the fill 0xA5 and has a canary behind its room, so a store at or past R (records, valid bytes),
R + 1 (offsets) or R * W (key bytes) shows; the 48-byte results byte for byte.

The kernels' constants as the shapes use them: 256 rows per block, so R in {0, 1, 255, 256, 257, 513} is no block, one partial
block, one full block, one full and one row, and two full and one row; a block's bytes leave in 16-byte stores and the last
block's tail byte by byte, so the widths 5, 10, 11, 16, 21, 55 and 88 give R * W mod 16 many residues and tails of 1 to 15
bytes.
"""
import ctypes
import json
import random
from fractions import Fraction

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from mojo_simdjson_amd.document_stream import FIELD_DTYPE
from tests import test_group_keys_math as tgm
from tests import test_tape_documents as ttd
from tests import test_validate_documents as tvd

pytestmark = pytest.mark.gpu

CANARY = 16
FILL = tgm.FILL
MSJ_CAPACITY, BAD_ARGUMENT = 1, -1
NUMBER, CODE, NULL_IS_GROUP = tgm.NUMBER, tgm.CODE, tgm.NULL_IS_GROUP
SIZES = (0, 1, 255, 256, 257, 513)


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
def gtw():
    return tgm.load_twin()


def filled(dev, n_bytes):
    """uint8[n_bytes + a canary] of the fill on the device, 16-byte aligned"""
    import torch

    t = torch.full((n_bytes + 16 * CANARY,), FILL, dtype=torch.uint8, device=dev.device)
    assert t.data_ptr() % 16 == 0
    return t


def with_canary(x, n_bytes):
    out = np.full(n_bytes + 16 * CANARY, FILL, dtype=np.uint8)
    raw = np.frombuffer(np.ascontiguousarray(x).tobytes(), dtype=np.uint8)
    out[:raw.size] = raw
    return out


def select_tensor(dev, R, code=0):
    return ttd.to_device(dev, np.frombuffer(bytes(tgm.select_result(R, code)), dtype=np.uint8))


def same(got, want, what):
    got = got.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, int(bad[0]), got[bad[:8]].tolist(), want[bad[:8]].tolist(), int(bad.size))


def run_bucket(dev, gtw, rows, R, width, origin=0, capacity=None, sel_code=0, in_place=False):
    """One call on the device against the twin over the whole of the record array -> the twin's tgm.Bucketed"""
    import torch

    rows = np.ascontiguousarray(rows, dtype=FIELD_DTYPE)
    capacity = len(rows) if capacity is None else capacity
    want = tgm.twin_bucket(gtw, rows, R, width, origin, capacity=capacity, sel_code=sel_code, in_place=in_place)
    assert want.rc == 0
    d_rows = filled(dev, 16 * len(rows))
    d_rows[:16 * len(rows)] = torch.from_numpy(np.frombuffer(rows.tobytes(), dtype=np.uint8).copy()).to(dev.device)
    d_out = d_rows if in_place else filled(dev, 16 * capacity)
    d_sel, d_res, d_osel = select_tensor(dev, R, sel_code), filled(dev, 48), filled(dev, 48)
    rc = dev.lib.msj_bucket_rows_device(dev.ctx, d_rows.data_ptr(), d_sel.data_ptr(), width, origin, 0, d_out.data_ptr(), capacity,
                                        d_res.data_ptr(), d_osel.data_ptr(), dev._stream())
    assert rc == 0
    torch.cuda.synchronize()
    same(d_res, with_canary(np.frombuffer(bytes(want.res), dtype=np.uint8), 48), "the result")
    same(d_osel, with_canary(np.frombuffer(bytes(want.out_sel), dtype=np.uint8), 48), "the output's select result")
    same(d_out, with_canary(want.out, 16 * (len(rows) if in_place else capacity)), "the records")
    if not in_place:
        same(d_rows, with_canary(rows, 16 * len(rows)), "the input")
    return want


def run_keys(dev, gtw, parts, R, capacity=None, bytes_capacity=None, sel_code=0):
    """One call on the device against the twin over the whole of the three arrays -> the twin's tgm.Keys"""
    import torch

    stride = len(parts[0].column)
    W = sum(p.width for p in parts)
    capacity = stride if capacity is None else capacity
    bytes_capacity = capacity * W if bytes_capacity is None else bytes_capacity
    want = tgm.twin_keys(gtw, parts, R, capacity=capacity, bytes_capacity=bytes_capacity, sel_code=sel_code)
    assert want.rc == 0
    columns = [ttd.to_device(dev, np.concatenate([p.column, np.zeros(1, dtype=p.column.dtype)])) for p in parts]   # (never an empty tensor)
    arr = tgm.part_array(parts, [c.data_ptr() for c in columns])
    d_off, d_valid, d_bytes = filled(dev, 8 * (capacity + 1)), filled(dev, capacity), filled(dev, bytes_capacity)
    d_sel, d_res = select_tensor(dev, R, sel_code), filled(dev, 48)
    rc = dev.lib.msj_group_keys_device(dev.ctx, arr, len(parts), stride, d_sel.data_ptr(), d_off.data_ptr(), d_valid.data_ptr(), d_bytes.data_ptr(),
                                       capacity, bytes_capacity, d_res.data_ptr(), dev._stream())
    assert rc == 0
    torch.cuda.synchronize()
    same(d_res, with_canary(np.frombuffer(bytes(want.res), dtype=np.uint8), 48), "the result")
    same(d_off, with_canary(want.offsets, 8 * (capacity + 1)), "the offsets")
    same(d_valid, with_canary(want.valid, capacity), "the valid bytes")
    same(d_bytes, with_canary(want.bytes, bytes_capacity), "the key bytes")
    return want


def bucket_rows_of(rng, n):
    values = tgm.EXTREME_INTS + tgm.EXTREME_DOUBLES + tgm.HOSTILE + tgm.tam.ODD_VALUES
    out = []
    for k in range(n):
        r = list(tgm.record(rng.choice(values) if rng.random() < 0.5 else rng.randint(-10**7, 10**7)))
        r[1] = 3 * k + 1
        out.append(tuple(r))
    return np.array(out, dtype=FIELD_DTYPE)


@pytest.mark.parametrize("R", SIZES)
def test_bucket_against_the_twin(dev, gtw, R):
    rng = random.Random(R)
    rows = bucket_rows_of(rng, R + 3)
    for width, origin in ((60000, 0), (1, -1), (2**63 - 1, tgm.INT64_MIN), (7, tgm.INT64_MAX)):
        want = run_bucket(dev, gtw, rows, R, width, origin)
        tgm.check_bucket(want, rows, R, width, origin, len(rows))
        run_bucket(dev, gtw, rows, R, width, origin, in_place=True)
    run_bucket(dev, gtw, rows, R, 60000, 0, capacity=R)   # the room exactly


def test_bucket_capacity_and_codes(dev, gtw):
    rows = bucket_rows_of(random.Random(1), 300)
    want = run_bucket(dev, gtw, rows, 300, 5, capacity=299)
    assert (want.res.code, want.res.n_rows, want.res.n_bucketed) == (MSJ_CAPACITY, 300, 0)
    want = run_bucket(dev, gtw, rows, 300, 5, sel_code=7)
    assert (want.res.code, want.res.n_rows) == (7, 0)
    want = run_bucket(dev, gtw, rows, 1 << 31, 5)
    assert (want.res.code, want.res.n_rows) == (MSJ_CAPACITY, 1 << 31)


@pytest.mark.parametrize("kinds", tgm.KIND_LISTS[:7], ids=lambda ks: "W%d" % sum(tgm.PART_BYTES[k] for k in ks))
@pytest.mark.parametrize("R", SIZES)
def test_keys_against_the_twin(dev, gtw, R, kinds):
    rng = random.Random(R * 100 + len(kinds))
    W = sum(tgm.PART_BYTES[k] for k in kinds)
    for flags in ([0] * len(kinds), [NULL_IS_GROUP] * len(kinds), None):   # off, on, and per part by chance
        parts = tgm.random_parts(rng, kinds, R + 2, flags)
        want = run_keys(dev, gtw, parts, R)
        tgm.check_keys(want, parts, R, R + 2, (R + 2) * W)
    run_keys(dev, gtw, tgm.random_parts(rng, kinds, R, None), R, capacity=R, bytes_capacity=R * W)   # every room exactly


def test_keys_every_number_of_parts(dev, gtw):
    rng = random.Random(8)
    for kinds in tgm.KIND_LISTS[7:]:
        run_keys(dev, gtw, tgm.random_parts(rng, kinds, 300), 257)


def test_keys_capacity_and_codes(dev, gtw):
    parts = tgm.random_parts(random.Random(2), [CODE, NUMBER], 300)
    W, R = 16, 257
    for kw in (dict(capacity=R - 1), dict(bytes_capacity=R * W - 1), dict(sel_code=9)):
        want = run_keys(dev, gtw, parts, R, **kw)
        assert want.res.code == (9 if "sel_code" in kw else MSJ_CAPACITY) and want.res.n_keys == 0 and want.res.bytes_len == 0
        assert (want.bytes == FILL).all() and (want.valid == FILL).all()
    assert run_keys(dev, gtw, parts, 301).res.code == MSJ_CAPACITY          # R > stride
    assert run_keys(dev, gtw, parts, 1 << 31).res.code == MSJ_CAPACITY


def test_argument_checks_in_their_order(dev):
    """Each call breaks one rule and, behind it, every later one: the code is the first rule's, and nothing is launched (the
    outputs keep their fill)"""
    import torch

    lib, ctx, s = dev.lib, dev.ctx, dev._stream()
    rows, out, codes = filled(dev, 16 * 8), filled(dev, 16 * 8), torch.zeros(8, dtype=torch.int32, device=dev.device)
    sel, res, osel = select_tensor(dev, 4), filled(dev, 48), filled(dev, 48)
    p = lambda t, shift=0: t.data_ptr() + shift
    bucket = lambda *a: lib.msj_bucket_rows_device(*a, s)
    # the bucket call: NULLs; NULL arrays with a capacity; width and flags; the capacity; overlap; the results; alignment
    assert bucket(None, p(rows), p(sel), 0, 0, 1, None, 8, p(res), p(osel)) == BAD_ARGUMENT
    assert bucket(ctx, None, p(sel), 0, 0, 1, p(out), 1 << 40, None, p(osel)) == BAD_ARGUMENT
    assert bucket(ctx, None, None, 0, 0, 1, p(out), 1 << 40, p(res), p(osel)) == BAD_ARGUMENT
    assert bucket(ctx, None, p(sel), 0, 0, 1, p(out), 1 << 40, p(res), p(osel)) == BAD_ARGUMENT       # NULL d_rows before the width
    assert bucket(ctx, p(rows), p(sel), 1, 0, 0, None, 8, p(res), p(osel)) == BAD_ARGUMENT
    assert bucket(ctx, p(rows), p(sel), 0, 0, 0, p(out), 1 << 40, p(res), p(osel)) == BAD_ARGUMENT    # the width before the capacity
    assert bucket(ctx, p(rows), p(sel), 1, 0, 1, p(out), 1 << 40, p(res), p(osel)) == BAD_ARGUMENT    # the flags likewise
    assert bucket(ctx, p(rows), p(sel), 1, 0, 0, p(rows, 16), 1 << 40, p(res), p(osel)) == MSJ_CAPACITY   # the capacity before the overlap
    assert bucket(ctx, p(rows), p(sel), 1, 0, 0, p(rows, 16), 8, p(res), p(sel)) == BAD_ARGUMENT      # the overlap
    assert bucket(ctx, p(rows), p(sel), 1, 0, 0, p(out, 8), 8, p(sel), p(osel)) == BAD_ARGUMENT       # d_result == a select result before alignment
    assert bucket(ctx, p(rows), p(sel), 1, 0, 0, p(out), 8, p(res), p(sel)) == BAD_ARGUMENT
    assert bucket(ctx, p(rows), p(sel), 1, 0, 0, p(out, 8), 8, p(res), p(osel)) == BAD_ARGUMENT
    assert bucket(ctx, p(rows, 8), p(sel), 1, 0, 0, p(out), 7, p(res), p(osel)) == BAD_ARGUMENT
    assert bucket(ctx, p(rows), p(sel), 1, 0, 0, p(out), 8, p(res, 4), p(osel)) == BAD_ARGUMENT
    assert bucket(ctx, None, p(sel), 1, 0, 0, None, 0, p(res), None) == 0                              # no room: no arrays needed
    torch.cuda.synchronize()
    got = _lib.MsjBucketRowsResult.from_buffer_copy(res[:48].cpu().numpy().tobytes())
    assert (got.code, got.n_rows) == (MSJ_CAPACITY, 4)
    res.fill_(FILL)

    off, valid, data = filled(dev, 8 * 9), filled(dev, 8), filled(dev, 16 * 8)
    table = (_lib.MsjKeyPart * 9)()

    def part(j, column, kind=NUMBER, flags=0):
        table[j].d_column, table[j].kind, table[j].flags = column, kind, flags

    def keys(parts=table, n=2, stride=8, sel_=None, off_=None, valid_=None, data_=None, capacity=8, res_=None):
        return lib.msj_group_keys_device(ctx, parts, n, stride, p(sel) if sel_ is None else sel_, p(off) if off_ is None else off_,
                                         p(valid) if valid_ is None else valid_, p(data) if data_ is None else data_, capacity, 16 * 8,
                                         p(res) if res_ is None else res_, s)
    part(0, p(rows)), part(1, p(codes), CODE)
    assert lib.msj_group_keys_device(None, table, 2, 8, p(sel), p(off), p(valid), p(data), 8, 128, p(res), s) == BAD_ARGUMENT
    assert keys(parts=None, n=0) == BAD_ARGUMENT
    part(1, p(codes), 3)
    assert keys(n=0) == BAD_ARGUMENT and keys(n=9) == BAD_ARGUMENT           # n_parts before the kinds
    part(0, None)
    assert keys() == BAD_ARGUMENT                                            # an unknown kind before a NULL column
    part(1, p(codes), CODE, 2)
    assert keys() == BAD_ARGUMENT                                            # an unknown flag likewise
    part(1, p(codes), CODE, NULL_IS_GROUP)
    assert keys(off_=0) == BAD_ARGUMENT                                      # a NULL column before the NULL outputs
    assert keys(stride=0, capacity=0, off_=0, valid_=0, data_=0) == 0        # no rows: no arrays needed
    torch.cuda.synchronize()
    got = _lib.MsjGroupKeysResult.from_buffer_copy(res[:48].cpu().numpy().tobytes())
    assert (got.code, got.n_rows, got.key_width) == (MSJ_CAPACITY, 4, 16)
    res.fill_(FILL)
    part(0, p(rows, 8))
    for kw in (dict(off_=0), dict(valid_=0), dict(data_=0)):
        assert keys(**kw) == BAD_ARGUMENT                                    # NULL outputs before alignment
    assert keys() == BAD_ARGUMENT                                            # records 16-byte
    part(0, p(rows)), part(1, p(codes, 2), CODE)
    assert keys() == BAD_ARGUMENT                                            # codes 4-byte
    part(1, p(codes), CODE)
    assert keys(data_=p(data, 8)) == BAD_ARGUMENT and keys(off_=p(off, 4)) == BAD_ARGUMENT
    assert keys(res_=p(res, 4)) == BAD_ARGUMENT and keys(sel_=p(sel, 4)) == BAD_ARGUMENT
    assert keys(res_=p(sel)) == BAD_ARGUMENT
    torch.cuda.synchronize()
    for t in (out, res, osel, off, valid, data):
        assert bool((t == FILL).all())
    assert keys() == 0


POINTERS = ["/ts", "/code", "/latency_ms"]


def chain_lines(n):
    rng = random.Random(77)
    out = []
    for k in range(n):
        ts = "2024-05-01T12:%02d:%02d.%03dZ" % (k % 7, rng.randrange(60), rng.randrange(1000)) if k % 13 else "1969-12-31T23:59:%02d.500Z" % (k % 60)
        code = rng.choice(["200", "200.0", "2e2", "404", "500", "503.5", '"x"', "null"])
        latency = rng.choice(["%d" % rng.randrange(10**6), "%d.25" % rng.randrange(1000), "9007199254740993", '"slow"'])
        doc = '{"ts":"%s","code":%s,"latency_ms":%s}' % (ts, code, latency)
        out.append(doc if k % 17 else '{"code":%s,"latency_ms":%s}' % (code, latency))
    return out


def test_chain_without_a_host_wait(dev):
    """select -> cast -> bucket -> keys -> msj_dictionary_device -> msj_aggregate_device with d_n_groups =
    &dictionary_result->n_distinct, every call behind the select enqueued with nothing waited for; then everything comes to the
    host and is compared with a Python dict of Fraction sums over json.loads of the same lines"""
    import datetime

    import torch

    from mojo_simdjson_amd.document_stream import DocumentStream

    lines = chain_lines(700)
    data = ("\n".join(lines) + "\n").encode()
    stream = DocumentStream(dev, tvd.upload(dev, data), len(data), window=1 << 20, select=POINTERS)
    (win,) = list(stream)
    D = win.n_documents
    assert D == len(lines)
    fields = win.d_fields
    _, d_ts, d_ts_sel = dev.cast_strings(win.d_window, win.length, fields[0].contiguous(), win.d_select, "timestamp", "ms", capacity=D, sync=False)
    _, d_minute, _ = dev.bucket_rows(d_ts, d_ts_sel, 60000, 0, capacity=D, d_out=d_ts, sync=False)
    d_kres, d_off, d_valid, d_bytes = dev.group_keys([fields[1].contiguous(), d_minute], win.d_select, capacity=D, sync=False)
    d_n_rows = d_kres[8:16].view(torch.int64)
    d_dres, d_codes, d_doff, d_dfirst, d_dbytes = dev.dictionary(d_off, d_bytes, d_valid, rows=D, d_n_rows=d_n_rows, bytes_len=D * 22, dict_capacity=D,
                                                                 dict_bytes_capacity=D * 22, sync=False)
    d_ares, d_groups = dev.aggregate(fields[2].contiguous(), win.d_select, d_codes, n_groups=0x7777, d_n_groups=d_dres[24:32].view(torch.int64),
                                     groups_capacity=D, sync=False)
    torch.cuda.synchronize()
    kres = _lib.MsjGroupKeysResult.from_buffer_copy(d_kres.cpu().numpy().tobytes())
    dres = _lib.MsjDictionaryResult.from_buffer_copy(d_dres.cpu().numpy().tobytes())
    ares = _lib.MsjAggregateResult.from_buffer_copy(d_ares.cpu().numpy().tobytes())
    assert (kres.code, kres.n_rows, kres.key_width, kres.bytes_len) == (0, D, 22, 22 * D) and dres.code == 0 and ares.code == 0
    G = int(dres.n_distinct)
    assert ares.n_groups == G and ares.n_rows == D

    # the plain-Python answer
    epoch = datetime.datetime(1970, 1, 1, tzinfo=datetime.timezone.utc)
    want, ungrouped = {}, 0
    for line in lines:
        doc = json.loads(line)
        code, ts = doc.get("code"), doc.get("ts")
        if isinstance(code, bool) or not isinstance(code, (int, float)) or ts is None:
            ungrouped += 1
            continue
        delta = datetime.datetime.fromisoformat(ts.replace("Z", "+00:00")) - epoch
        ms = (delta.days * 86400 + delta.seconds) * 1000 + delta.microseconds // 1000
        key = (Fraction(code), ms // 60000 * 60000)
        n, total = want.setdefault(key, [0, Fraction(0)])
        v = doc["latency_ms"]
        want[key] = [n + 1, total + (Fraction(v) if isinstance(v, (int, float)) else 0)]
    assert ungrouped > 0 and kres.n_keys == D - ungrouped and ares.n_ungrouped == ungrouped and len(want) == G
    gtw = tgm.load_twin()
    off, key_bytes = d_doff.cpu().tolist(), d_dbytes.cpu().numpy().tobytes()
    rec = d_groups.cpu().numpy()[:48 * G].view("<u8").reshape(G, 6)
    tags = d_groups.cpu().numpy()[:48 * G].reshape(G, 48)[:, 40]
    got = {}
    for g in range(G):
        code, minute = tgm.decode_key(gtw, [NUMBER, NUMBER], key_bytes[off[g]:off[g + 1]])
        total = int(rec[g, 2]) - ((1 << 64) if tags[g] == ord("l") and int(rec[g, 2]) >> 63 else 0) if tags[g] == ord("l") else \
            Fraction(tgm.bits_double(int(rec[g, 2]))) if tags[g] == ord("d") else 0
        got[(Fraction(code), minute)] = [int(rec[g, 0]), Fraction(total)]
    assert set(got) == set(want)
    # a group's 'l' sum is exact.  A 'd' sum is the exact sum of the values cut 95 binary places below the largest, rounded once:
    # every value here is positive, so the total is at least the largest value and both errors stay below 2^-52 of it
    for key, (n, total) in want.items():
        assert got[key][0] == n, key
        assert got[key][1] == total or abs(got[key][1] - total) <= abs(total) * Fraction(1, 2**52), (key, got[key], total)
    assert any(minute < 0 for _, minute in got)
