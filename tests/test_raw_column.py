"""A selected value's JSON text as a column on the device (msj_raw_column_device, csrc/raw_column_kernel.hip).

Expected values come from the host twin of the same arithmetic (tests/raw_column_math_host.cpp), which
tests/test_raw_column_math.py holds against a yardstick written in Python.  Device output is compared with the twin over
the WHOLE d_offsets, d_valid and d_bytes arrays (both start from the same fill, with 64 bytes of canary behind each
capacity, so a store the twin does not make shows).  Records come from the real chain (shard, stage2_prep, documents,
number_values, select_documents, array_column, select_elements, object_entries) -- the twin then runs over the arrays the
device made, downloaded -- and, where a shape is wanted that the chain cannot give, hand-made and uploaded.

The kernels' constants (csrc/raw_column_kernel.hip) are named below as the shapes use them.
"""

import json

import numpy as np
import pytest

from mojo_simdjson_amd import synth
from mojo_simdjson_amd.document_stream import FIELD_DTYPE
from tests import helpers
from tests import test_number_math as tnm
from tests import test_raw_column_math as trm
from tests import test_select_documents as tsd
from tests import test_tape_documents as ttd
from tests import test_tape_documents_math as tdk
from tests import test_validate_documents as tvd

pytestmark = pytest.mark.gpu

B = 256                     # kRows: rows per workgroup of rc_lengths / rc_copy
ROW_GRID = 4096 * B         # kGridBlocks = 4096 blocks of kRows rows, `v += gridDim.x`
SCAN_CHUNK = 1024           # wave_ops.h, scan_in_place: blocks (of rows, of tokens) per chunk of the running sum
TOK_BLOCK = 1024            # kTokBlock: tokens per workgroup of rc_tokens
TOK_GRID = 2048 * TOK_BLOCK  # kTokGrid = 2048 blocks of kTokBlock tokens, `v += gridDim.x`
LONG_ROW = 16384            # kLongRow: a row of MORE bytes than this is on the list of long rows, copied by the whole grid
LONG_CAP = 1024             # kLongCap: entries of that list; a long row past it is carried by its block
PIECE = 16384               # kPiece: bytes of a long row one workgroup copies at a time
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
        self.rtwin = trm.load_twin()
        self._paths = {}

    def paths(self, pointers):
        key = tuple(pointers)
        if key not in self._paths:
            self._paths[key] = self.dev.compile_paths(pointers)
        return self._paths[key]


class OnDevice:
    """Host arrays (trm.Arrays) uploaded, padded so that no tensor is empty; d_match is not read by the call: zeros"""

    def __init__(self, dev, a):
        pad = lambda x, dt: np.concatenate([np.ascontiguousarray(x, dtype=dt), np.zeros(8, dtype=dt)])
        self.dev, self.length, self.n = dev, a.length, a.n
        self.d_buf = ttd.to_device(dev, np.frombuffer(a.data + b"\0" * 16, dtype=np.uint8))
        self.d_idx, self.d_end = ttd.to_device(dev, pad(a.idx, np.uint32)), ttd.to_device(dev, pad(a.end, np.uint32))
        self.d_type, self.d_flags = ttd.to_device(dev, pad(a.typ, np.uint8)), ttd.to_device(dev, pad(a.flags, np.uint8))
        self.d_match = ttd.to_device(dev, np.zeros(a.n + 8, dtype=np.uint32))


def chain_of(env, data, verdicts=False):
    """The real chain over `data` and what the twin needs of it, downloaded -> (FromChain, trm.Arrays)"""
    c = tsd.FromChain(env.dev, data, False, verdicts)
    host = lambda t, dt: t.cpu().numpy().view(dt)[:c.n].copy()
    return c, trm.Arrays(data, host(c.d_idx, np.uint32), host(c.d_type, np.uint8), host(c.d_end, np.uint32), host(c.d_flags, np.uint8))


def select(env, c, pointers, room=3):
    """msj_select_documents_device over the chain -> (d_fields (n_paths, capacity, 2), d_sel, D)"""
    from mojo_simdjson_amd import _lib

    d_docs = _lib.MsjDocumentsResult.from_buffer_copy(c.d_docs.cpu().numpy().tobytes())
    D = int(d_docs.n_complete)
    d_sel, d_fields = env.dev.select_documents(env.paths(pointers), c.d_buf, c.length, c.d_idx, c.n, c.d_type, c.d_depth, c.d_match, c.d_end,
                                               c.d_flags, c.d_first, c.d_docs, d_numbers=c.d_numbers, numbers_capacity=c.ncap,
                                               d_numbers_result=c.d_num, d_verdicts=c.d_verdicts, capacity=D + room, sync=False)
    return d_fields, d_sel, D


def records_of(d_rows, R):
    return np.ascontiguousarray(d_rows[:R].cpu().numpy()).view(FIELD_DTYPE).reshape(-1).copy()


def upload_records(dev, records, code=0):
    """Hand-made records as a (rows + 1, 2) tensor (never empty) and a select result that counts them"""
    rows = np.concatenate([np.ascontiguousarray(records), np.zeros(1, dtype=FIELD_DTYPE)])
    d_rows = ttd.to_device(dev, rows).reshape(-1, 2)
    d_sel = ttd.to_device(dev, np.frombuffer(bytes(trm.select_result(len(records), code)), dtype=np.uint8))
    return d_rows, d_sel


def device_raw(dev, a, d_rows, d_sel, want, shift=0):
    """msj_raw_column_device with the twin's capacities and flags, its arrays filled like the twin's with their canaries;
    shift: d_bytes starts that many bytes off a 16-byte boundary -> trm.Column"""
    import torch

    offsets, valid, data = trm.filled(want.capacity, want.bytes_capacity, want.data is None)
    d_off = torch.from_numpy(offsets.view(np.int64)).to(dev.device)
    d_valid = torch.from_numpy(valid).to(dev.device)
    d_all = torch.from_numpy(np.concatenate([np.full(shift, trm.FILL, dtype=np.uint8), data])).to(dev.device) if data is not None else None
    d_bytes = d_all[shift:] if data is not None else None
    res, _, _, _ = dev.raw_column(a.d_buf, a.length, a.d_idx, a.n, a.d_type, a.d_match, a.d_end, a.d_flags, d_rows, d_sel, d_offsets=d_off,
                                  d_valid=d_valid, d_bytes=d_bytes, capacity=want.capacity, bytes_capacity=want.bytes_capacity,
                                  compact=bool(want.flags), text=data is not None)
    if data is not None:
        assert bool((d_all[:shift] == trm.FILL).all())
    return trm.Column(res, d_off.cpu().numpy().view(np.uint64), d_valid.cpu().numpy(), d_bytes.cpu().numpy() if data is not None else None,
                      want.capacity, want.bytes_capacity, want.flags)


def same(got, want, where=None):
    """The device's result and every array are the twin's, fill and canary included"""
    assert got.summary() == want.summary(), (where, got.summary(), want.summary())
    for name in ("offsets", "valid", "data"):
        x, y = getattr(got, name), getattr(want, name)
        if y is None:
            assert x is None
            continue
        bad = np.nonzero(x != y)[0]
        assert bad.size == 0, (where, name, int(bad[0]), x[bad[:4]].tolist(), y[bad[:4]].tolist(), bad.size)


def check(env, a, host, d_rows, d_sel, records, forms=(False, True), layouts=(True, False), shift=0, where=None, **kw):
    """The device against the twin: verbatim and compact, layout-only and with the bytes -> the last twin Column per form"""
    out = {}
    for compact in forms:
        for layout_only in layouts:
            want = trm.twin_raw(env.rtwin, host, records, compact=compact, layout_only=layout_only, **kw)
            same(device_raw(env.dev, a, d_rows, d_sel, want, shift), want, (where, compact, layout_only))
        out[compact] = want
    return out


def text(k, n):
    return "".join(chr(ord("a") + (k + j) % 26) for j in range(n))


def line(k, value=None):
    """Document k of a mixed column: strings of 0 .. 40 characters, numbers, containers, atoms, a missing key"""
    kinds = [text(k, k % 41), k * 37, {"a": [k, "x y"], "b": {}}, [k, [k, "}"]], True, None, -0.5]
    if value is None and k % 8 == 7:
        return b'{"t":%d}' % k
    v = kinds[k % 8 % 7] if value is None else value
    return json.dumps({"s": v}, separators=(",", ":")).encode()


def mixed(env, lines, pointer="/s"):
    data = tdk.join(lines, b"\n")
    c, host = chain_of(env, data)
    d_fields, d_sel, D = select(env, c, [pointer])
    assert D == len(lines)
    return c, host, d_fields[0], d_sel, records_of(d_fields[0], D)


def string_of(n):
    """A value whose text has exactly n bytes"""
    return text(n, n - 2)


@pytest.mark.parametrize("n", [1, B - 1, B, B + 1, 2 * B + 1])
def test_row_counts(env, n):
    """1, B - 1, B, B + 1 and 2 B + 1 rows of every kind from the real chain; d_bytes on and off a 16-byte boundary."""
    c, host, d_rows, d_sel, records = mixed(env, [line(k) for k in range(n)])
    for shift in (0, 5):
        out = check(env, c, host, d_rows, d_sel, records, shift=shift, capacity=n + 3, where=(n, shift))
    assert out[False].rows() == out[True].rows() and out[False].res.n_values == n - n // 8
    rows = out[False].rows()
    assert rows[0] == b'""' and (n < 3 or rows[2] == b'{"a":[2,"x y"],"b":{}}')


def test_empty_rows_at_block_ends_and_all_invalid(env):
    """Rows of length 0 -- a missing key, hand-made records that fail the row test -- on the first and last rows of two
    blocks, between rows with bytes; then 2 B + 1 rows that are all invalid: no byte, nothing of d_bytes touched."""
    lines = [line(k, value=text(k, 1 + k % 30)) for k in range(2 * B + 9)]
    for k in (0, 1, B - 2, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 8):
        lines[k] = b'{"t":0}'
    c, host, d_rows, d_sel, records = mixed(env, lines)
    out = check(env, c, host, d_rows, d_sel, records)
    assert out[False].res.n_values == 2 * B and out[False].rows()[0] is None and out[False].rows()[2] == b'"cde"'
    kinds = [lambda k: trm.record(0xFFFFFFFF, "", code=20), lambda k: trm.record(host.n, "l"), lambda k: trm.record(host.n + k, '"'),
             lambda k: trm.record(k % host.n, "{", bits=k % host.n - k % 2), lambda k: trm.record(k % host.n, "[", bits=host.n + k % 2)]
    bad = np.concatenate([kinds[k % 5](k) for k in range(2 * B + 1)])   # a code; a token at and past n; a partner at or below the token, at or past n
    d_bad, d_bad_sel = upload_records(env.dev, bad)
    out = check(env, c, host, d_bad, d_bad_sel, bad, bytes_capacity=32)
    assert out[True].summary() == (0, 1, 2 * B + 1, 0, 0, 0, 2 * B + 1 - 103) and out[True].untouched(2 * B + 1, 0)


@pytest.mark.parametrize("at", [3, B - 1, B])
def test_rows_around_the_threshold(env, at):
    """Rows of kLongRow - 1, kLongRow and kLongRow + 1 bytes between short ones: the last is copied by rc_long, the others
    by their block, whose range then covers what several blocks of their neighbours write.  The long row is row 3, a block's
    last row and a block's first row, with a long container behind it."""
    lines = [line(k) for k in range(B + 40)]
    for j, size in enumerate((LONG_ROW + 1, LONG_ROW, LONG_ROW - 1)):
        lines[(at + 20 * j) % (B + 40)] = line(0, value=string_of(size))
    box = [string_of(LONG_ROW - 2), 1, {"k": [None]}]
    lines[at + 1] = line(0, value=box)
    c, host, d_rows, d_sel, records = mixed(env, lines)
    out = check(env, c, host, d_rows, d_sel, records, shift=at % 7, where=at)
    sizes = sorted(len(r) for r in out[False].rows() if r is not None)[-4:]
    assert sizes == [LONG_ROW - 1, LONG_ROW, LONG_ROW + 1, len(json.dumps(box, separators=(",", ":")))] and sizes[3] > LONG_ROW + 1


@pytest.mark.parametrize("extra", [-1, 0, 1])
def test_long_row_list(env, extra):
    """kLongCap - 1, kLongCap and kLongCap + 1 long rows: hand-made records that all name one container of kLongRow + 8
    bytes, short rows between them.  The row that finds the list full is carried by its block: the same bytes."""
    lines = [line(0, value=[string_of(LONG_ROW), 1, 2, 3]), line(1), line(2)]
    c, host, d_fields, _, chain_records = mixed(env, lines)
    big, short = chain_records[0:1], chain_records[2:3]
    records = np.concatenate([big if k % 2 == 0 else short for k in range(2 * (LONG_CAP + extra))])
    d_rows, d_sel = upload_records(env.dev, records)
    forms = (False, True) if extra == 1 else (False,)
    out = check(env, c, host, d_rows, d_sel, records, forms=forms, layouts=(False,), where=extra)
    assert out[False].res.total_bytes == (LONG_CAP + extra) * (LONG_ROW + 8 + len(b'{"a":[2,"x y"],"b":{}}'))


def test_row_grid_and_scan_wraps(env):
    """ROW_GRID + 300 hand-made short records over a small window: rows past the grid x 256 of rc_lengths / rc_copy
    (`v += gridDim.x`) and 4 097 block sums, the fifth chunk of rc_scan's running sum."""
    c, host, _, _, chain_records = mixed(env, [line(k) for k in range(16)])
    R = ROW_GRID + 300
    assert (R + B - 1) // B > 4 * SCAN_CHUNK
    records = np.tile(chain_records, R // 16 + 1)[:R].copy()
    records[ROW_GRID - 1], records[ROW_GRID], records[R - 1] = chain_records[2], chain_records[3], chain_records[2]
    d_rows, d_sel = upload_records(env.dev, records)
    out = check(env, c, host, d_rows, d_sel, records, layouts=(False,))
    assert out[True].rows()[R - 1] == b'{"a":[2,"x y"],"b":{}}'


def test_token_grid_and_scan_wraps(env):
    """A window of TOK_GRID + 4 100 tokens, [1,1,...,1] with arrays written down by hand: compact rows past the grid of
    rc_tokens and in the third chunk of rc_tscan's running sum; the root, one row of 2 MiB whose tokens the copy searches."""
    n = TOK_GRID + 4100 + 1
    assert n % 2 == 1 and n // TOK_BLOCK + 1 > 2 * SCAN_CHUNK
    data = np.full(n, ord(","), dtype=np.uint8)
    data[1::2] = ord("1")
    data[0], data[-1] = ord("["), ord("]")
    idx = np.arange(n, dtype=np.uint32)
    flags = np.where(data == ord("1"), 4, 0).astype(np.uint8)
    host = trm.Arrays(data.tobytes(), idx, data, np.where(flags == 4, idx + 1, 0), flags)
    a = OnDevice(env.dev, host)
    tokens = [1, TOK_BLOCK - 1, TOK_BLOCK, SCAN_CHUNK * TOK_BLOCK - 1, SCAN_CHUNK * TOK_BLOCK + 1, TOK_GRID - 1, TOK_GRID + 1, TOK_GRID + 4099, n - 2]
    records = np.concatenate([trm.record(0, "[", bits=n - 1)] + [trm.record(t, "l") for t in tokens] + [trm.record(n - 1, "l"), trm.record(n, "l")])
    d_rows, d_sel = upload_records(env.dev, records)
    out = check(env, a, host, d_rows, d_sel, records, layouts=(False,))
    assert out[True].res.total_bytes == n + len(tokens) + 1 and out[True].res.n_other == 1 and out[True].rows()[0] == data.tobytes()


def test_capacities(env):
    """bytes_capacity one short, exact and 0: the offsets complete, the bytes clipped, the canary intact; capacity R - 1:
    nothing but the result; a select call that ran out of capacity itself: its code; no row at all."""
    import torch

    lines = [line(k) for k in range(B + 5)]
    lines[3], lines[B] = line(0, value=string_of(LONG_ROW + 100)), line(0, value=[string_of(700), {"k": 1}])
    c, host, d_rows, d_sel, records = mixed(env, lines)
    R = len(lines)
    for compact in (False, True):
        f = 1 if compact else 0
        total = int(trm.twin_raw(env.rtwin, host, records, compact=compact, layout_only=True).res.total_bytes)
        for kw in (dict(bytes_capacity=total - 1), dict(bytes_capacity=total), dict(bytes_capacity=0), dict(bytes_capacity=LONG_ROW // 2), dict(bytes_capacity=PIECE + 5),
                   dict(capacity=R - 1, bytes_capacity=total), dict(capacity=R + 300, bytes_capacity=total + 100)):
            want = trm.twin_raw(env.rtwin, host, records, compact=compact, **kw)
            same(device_raw(env.dev, c, d_rows, d_sel, want, shift=3), want, (compact, kw))
            if "capacity" not in kw:
                assert want.res.code == (MSJ_CAPACITY if kw["bytes_capacity"] < total else 0) and want.res.total_bytes == total
                assert want.untouched(R, min(total, kw["bytes_capacity"]))
        over = trm.twin_raw(env.rtwin, host, records, compact=compact, capacity=R - 1, bytes_capacity=total)
        assert over.summary() == (MSJ_CAPACITY, f, R, 0, 0, 0, 0) and over.untouched(-1, 0)
        # the real select call with one record too few: its result has MSJ_CAPACITY, and so has the column's
        d_fields, d_short, _ = select(env, c, ["/s"], room=-1)
        want = trm.twin_raw(env.rtwin, host, records, compact=compact, sel_code=MSJ_CAPACITY, bytes_capacity=total)
        got = device_raw(env.dev, c, d_fields[0], d_short, want)
        same(got, want)
        assert got.summary() == (MSJ_CAPACITY, f, 0, 0, 0, 0, 0) and got.untouched(-1, 0)
        _, d_sel0 = upload_records(env.dev, records[:0])
        want = trm.twin_raw(env.rtwin, host, records, R=0, compact=compact, capacity=4, bytes_capacity=8)
        same(device_raw(env.dev, c, d_rows, d_sel0, want), want)
        assert want.offsets[0] == 0 and want.summary() == (0, f, 0, 0, 0, 0, 0)
    torch.cuda.synchronize()


def test_bad_arguments(env):
    """Each is refused with nothing launched, in the header's order: the outputs keep what was in them."""
    import torch

    dev = env.dev
    c, host, d_rows, d_sel, records = mixed(env, [line(0, value="a"), line(1, value=[1])])
    d_rows = d_rows.contiguous()
    sent = torch.full((8,), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    off = torch.full((8,), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    val = torch.full((16,), 0x5A, dtype=torch.uint8, device=dev.device)
    out = torch.full((32,), 0x5A, dtype=torch.uint8, device=dev.device)

    def call(**kw):
        p = dict(buf=c.d_buf.data_ptr(), len=c.length, idx=c.d_idx.data_ptr(), n=c.n, typ=c.d_type.data_ptr(), match=c.d_match.data_ptr(),
                 end=c.d_end.data_ptr(), flg=c.d_flags.data_ptr(), rows=d_rows.data_ptr(), sel=d_sel.data_ptr(), off=off.data_ptr(),
                 val=val.data_ptr(), cap=2, out=out.data_ptr(), room=16, flags=0, res=sent.data_ptr())
        p.update(kw)
        return dev.lib.msj_raw_column_device(dev.ctx, p["buf"], p["len"], p["idx"], p["n"], p["typ"], p["match"], p["end"], p["flg"], p["rows"],
                                             p["sel"], p["off"], p["val"], p["cap"], p["out"], p["room"], p["flags"], p["res"], dev._stream())

    for name in ("res", "sel", "buf", "idx", "typ", "end", "flg", "rows", "off", "val", "out"):
        assert call(**{name: None}) == BAD_ARGUMENT, name
    assert call(flags=2) == BAD_ARGUMENT and call(flags=3) == BAD_ARGUMENT
    assert call(len=(1 << 32) + 16) == MSJ_CAPACITY and call(n=1 << 31) == MSJ_CAPACITY
    # the order: a missing array wins over the size, the size over an off-grid pointer
    assert call(len=(1 << 32) + 16, out=None) == BAD_ARGUMENT and call(n=1 << 31, rows=d_rows.data_ptr() + 8) == MSJ_CAPACITY
    for name, base, step in (("rows", d_rows, 8), ("off", off, 4), ("sel", d_sel, 4), ("res", sent, 4), ("idx", c.d_idx, 2), ("end", c.d_end, 1),
                             ("match", c.d_match, 2)):
        assert call(**{name: base.data_ptr() + step}) == BAD_ARGUMENT, name
    torch.cuda.synchronize()
    assert bool((sent == tvd.SENTINEL).all()) and bool((off == tvd.SENTINEL).all()) and bool((val == 0x5A).all()) and bool((out == 0x5A).all())
    assert dev.lib.msj_raw_column_workspace_bytes(0, 0, 0) > 0
    assert dev.lib.msj_raw_column_workspace_bytes(1000, 10, 1) >= dev.lib.msj_raw_column_workspace_bytes(1000, 10, 0) + 8 * 1001
    # d_match NULL (it is not read), unaligned d_valid / d_bytes, the layout-only form, no token array with n == 0, and no
    # capacity at all with NULL arrays (R > 0: MSJ_CAPACITY in the result)
    assert call(match=None, val=val.data_ptr() + 1, out=out.data_ptr() + 3, room=8, flags=1) == 0 and call(out=None, room=0) == 0
    torch.cuda.synchronize()
    assert out.cpu().numpy()[3:11].tobytes() == b'"a"[1]\x5a\x5a' and val.cpu().numpy()[1:3].tolist() == [1, 1] and off.cpu().numpy()[:3].tolist() == [0, 3, 6]
    assert call(rows=None, off=None, val=None, cap=0, out=None, room=0) == 0
    torch.cuda.synchronize()
    assert sent.cpu().numpy()[:6].tolist() == [MSJ_CAPACITY, 2, 0, 0, 0, 0]
    assert call(idx=None, typ=None, end=None, flg=None, n=0, flags=1) == 0
    torch.cuda.synchronize()
    assert sent.cpu().numpy()[:6].tolist() == [1 << 32, 2, 0, 0, 0, 2]   # code 0, flags 1; both rows fail the row test


@pytest.mark.parametrize("name", ["pretty4", "minified"])
def test_synthetic_window(env, name):
    """~48 KiB of the synthetic workload as one document: the root, a container path and, through array_column, the elements
    of a list column, each against the twin.  pretty4: the compact rows decode to what the verbatim ones do and hold no line
    break; minified: compact equals verbatim on the device."""
    data = synth.workload(name, 48 << 10).tobytes()
    c, host = chain_of(env, data)
    d_fields, d_sel, D = select(env, c, ["", "/statuses", "/search_metadata"])
    assert D == 1
    d_esel = ttd.to_device(env.dev, np.zeros(48, dtype=np.uint8))
    res, _, _, d_elements, _ = env.dev.array_column(c.d_idx, c.n, c.d_type, c.d_depth, c.d_match, c.d_end, c.d_flags, c.d_first, c.d_docs, d_fields, 1,
                                                    d_sel, d_numbers=c.d_numbers, numbers_capacity=c.ncap, d_numbers_result=c.d_num,
                                                    d_elements_select=d_esel)
    assert res.code == 0 and res.n_elements > 10
    for d_rows, sel, R in ((d_fields[0], d_sel, 1), (d_fields[1], d_sel, 1), (d_elements, d_esel, int(res.n_elements))):
        records = records_of(d_rows, R)
        assert all(r["code"] == 0 for r in records)
        out = check(env, c, host, d_rows, sel, records, layouts=(False,), where=(name, R))
        v, k = out[False].rows(), out[True].rows()
        if name == "minified":
            assert v == k
        else:
            assert all(json.loads(x) == json.loads(y) and len(y) < len(x) and b"\n" not in y for x, y in zip(v, k))
    assert v[0].startswith(b"{") and len(v) == int(res.n_elements) and out[False].res.n_containers == len(v)


def test_document_stream_raw(env):
    """DocumentStream(select=[...]) over two windows and more: Window.raw, ListColumn.raw, ElementFields.raw and
    MapColumn.values().raw(), verbatim and compact, sliced back on the host, decode to what values() / to_python() give for
    the same rows; a row that is not valid has no bytes.  The documents are pretty-printed every other line."""
    import torch
    from mojo_simdjson_amd.document_stream import DocumentStream

    dev = env.dev
    docs = [{"id": k, "tags": ["a%d" % k, {"x": [k, None]}, [1, 2.5], "q\"\\"], "attrs": {"color": "red %d" % k, "n": {"z": [k]}, "e": []},
             "items": [{"sku": "s%d" % j, "dims": {"w": j, "h": [k, {"d": "}"}]}} for j in range(k % 3)]} for k in range(120)]
    docs[7] = {"id": "seven", "tags": 5, "attrs": [1], "items": {}}
    lines = [json.dumps(d, indent=None if k % 2 else 2).encode() for k, d in enumerate(docs)]
    lines[9] = b'{"id":9,"tags":[tru]}'
    data = b"\n".join(lines) + b"\n"
    pointers = ["", "/id", "/tags", "/attrs", "/items"]
    windows = 0

    def rows_of(column, n):
        offsets, out, valid = column
        assert offsets.dtype == torch.int64 and out.dtype == torch.uint8 and valid.dtype == torch.bool and offsets.is_cuda and out.is_cuda
        assert offsets.shape == (n + 1,) and valid.shape == (n,)
        off, raw, ok = offsets.cpu().tolist(), out.cpu().numpy().tobytes(), valid.cpu().tolist()
        assert off[-1] == len(raw)
        assert all(ok[k] or off[k] == off[k + 1] for k in range(n))
        return [raw[off[k]:off[k + 1]] if ok[k] else None for k in range(n)]

    def agree(verbatim, compact, values, what):
        assert len(verbatim) == len(compact) == len(values), what
        for v, c, want in zip(verbatim, compact, values):
            if v is None:
                assert c is None and want is None, what
                continue
            assert json.loads(v) == want and json.loads(c) == want and len(c) <= len(v) and b"\n" not in c, (what, v[:60])

    flat = lambda rows: [x for r in rows if r is not None for x in r]
    seen = 0
    for win in DocumentStream(dev, tvd.upload(dev, data), len(data), window=8192, select=pointers):
        D = win.n_documents
        for p in pointers:
            room = 1 if windows % 2 else None   # (1: the buffer has to grow)
            agree(rows_of(win.raw(p, bytes_capacity=room), D), rows_of(win.raw(p, compact=True, bytes_capacity=room), D), win.values(p), p)
        assert [json.loads(x) for x in rows_of(win.raw(""), D) if x is not None] == [d for k, d in enumerate(docs[seen:seen + D]) if seen + k != 9]
        tags = win.elements("/tags")
        agree(rows_of(tags.raw(), tags.n_elements), rows_of(tags.raw(compact=True), tags.n_elements), flat(tags.to_python()), "tags")
        fields = win.elements("/items").select(["/sku", "/dims", "/dims/h"])
        for p in ("/sku", "/dims", "/dims/h"):
            agree(rows_of(fields.raw(p), fields.n_elements), rows_of(fields.raw(p, compact=True), fields.n_elements), fields.values(p), p)
        attrs = win.entries("/attrs")
        values = attrs.values()
        agree(rows_of(values.raw(), attrs.n_entries), rows_of(values.raw(compact=True), attrs.n_entries), flat(values.to_python()), "attrs")
        keys = rows_of(attrs.keys(), attrs.n_entries)
        assert set(keys) <= {b"color", b"n", b"e"}
        seen += D
        windows += 1
    assert windows >= 2 and seen == len(docs)
