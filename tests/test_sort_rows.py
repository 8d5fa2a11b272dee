"""Rows by exact numeric order on the device (msj_sort_rows_device, csrc/sort_rows_kernel.hip).

Expected values come from the host twin of the same arithmetic (tests/sort_rows_math_host.cpp: the header's key and a serial
stable sort), which tests/test_sort_rows_math.py holds against the definition written in Python with Fraction.  Device output
is compared with the twin byte for byte: d_order over its WHOLE tensor (both start from the fill 0xA5, with a canary behind
the room, so a store at or past K shows), the 48-byte result and d_order_select.  Every comparison runs in all three modes of
msj_debug_set_sort_mode -- the path chosen on the device, always the full sort, always the selection carried to the key's
last digit -- which have to write the same bytes.  Records are made on the host and uploaded; the end-to-end test runs the
real chain through DocumentStream.

The kernel's constants (csrc/sort_rows_kernel.hip) are named below as the shapes use them.
"""
import datetime
import json

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from mojo_simdjson_amd.document_stream import FIELD_DTYPE
from tests import test_aggregate_math as tam
from tests import test_sort_rows_math as tsm
from tests import test_string_column_math as tcm
from tests import test_tape_documents as ttd
from tests import test_validate_documents as tvd

pytestmark = pytest.mark.gpu

B = 256            # kRows: rows per workgroup of the kernels with a lane per row
T = 1024           # kTile: keys per block per pass
S = 1024           # kScan: block sums per scan chunk
CANARY = 16        # entries behind d_order's room
MODES = (0, 1, 2)
MSJ_CAPACITY, BAD_ARGUMENT = 1, -1
FILL, FILL32 = tsm.FILL, tsm.FILL32
DESC, VALUES_ONLY = tsm.DESC, tsm.VALUES_ONLY
L, D = tam.L, tam.D
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, S * T + 1]


@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    d = Stage1Device(0)
    yield d
    d.set_sort_mode()
    d.close()


@pytest.fixture(scope="module")
def stw():
    return tsm.load_twin()


def struct_to_device(dev, s):
    import torch

    return torch.from_numpy(np.frombuffer(bytes(s), dtype=np.uint8).copy()).to(dev.device)


# ---- columns, made with numpy: a million records take no Python loop -----------------------------------------------------------

def column(bits, types, codes=None, flags=None):
    col = np.zeros(len(bits), dtype=FIELD_DTYPE)
    col["bits"], col["type"] = np.asarray(bits).astype(np.uint64), types
    if codes is not None:
        col["code"] = codes
    if flags is not None:
        col["flags"] = flags
    return col


def ints(values):
    return column(np.asarray(values, dtype=np.int64).view(np.uint64), L)


def doubles(values):
    return column(np.asarray(values, dtype=np.float64).view(np.uint64), D)


def pick(mask, a, b):
    """a where the mask is set, else b"""
    out = b.copy()
    out[mask] = a[mask]
    return out


def without_values(col, every=4, phase=1):
    """Every `every`-th row a row without a value, of changing kinds"""
    col = col.copy()
    k = np.arange(len(col))
    hit = k % every == phase
    col["type"][hit & (k % 3 == 0)] = ord("n")
    col["code"][hit & (k % 3 == 1)] = 20
    col["flags"][hit & (k % 3 == 2)] = tam.NO_BITS
    return col


def one_digit_column(n, digit, rng):
    """Keys that differ in exactly one of the eleven digits (sort_rows_math.h): lo's 8 + 2 bits (ints next to 2^62, whose
    last place is 2^10), a byte of hi (the double's pattern), the null bit"""
    x = rng.integers(0, 4 if digit == 1 else 256, n, dtype=np.uint64)
    if digit == 10:      # (a row without a value has hi = 0 as well: the null bit never differs alone)
        return without_values(ints(np.full(n, 7)), 2, 0)
    if digit < 2:
        return ints((np.uint64(2**62) + (x << np.uint64(8 * digit))).view(np.int64))
    if digit == 9:       # (the pattern's top byte holds the exponent's top: 0x40 .. 0x7E stays finite)
        return column((np.uint64(0x40) + x % np.uint64(0x3F)) << np.uint64(56), D)
    return column(np.uint64(0x4000000000000000) + (x << np.uint64(8 * (digit - 2))), D)


def columns_of(n, seed):
    """name -> column for a size: the kinds of column the call has to get right"""
    rng = np.random.default_rng(seed)
    k = np.arange(n, dtype=np.int64)
    out = {
        "all equal": ints(np.full(n, 42)),
        "ascending": ints(k * 3 - n),
        "reversed": doubles((n - k) * 0.5),
        "every digit value": pick(k % 2 == 0, ints(rng.integers(-2**63, 2**63 - 1, n)), column(rng.integers(0, 2**64, n, dtype=np.uint64) & np.uint64(0xFFEFFFFFFFFFFFFF), D)),      # (finite)
        "int / double alternating": pick(k % 2 == 0, ints(k // 4), doubles((k // 4).astype(np.float64))),
        "negatives and subnormals": pick(k % 3 == 0, ints(-(k % 50)), column(rng.integers(0, 2**20, n, dtype=np.uint64) | (k % 2).astype(np.uint64) << np.uint64(63), D)),
        "every fourth without a value": without_values(ints(rng.integers(-1000, 1000, n)), 4, 1),
        "no value at all": column(k.astype(np.uint64), ord('"')),
        "beside 2^53": pick(k % 2 == 0, ints(2**53 + (k % 7)), doubles(2.0**53 + 2 * (k % 5))),
    }
    return out if n <= 2 * T + 1 else {name: out[name] for name in ("all equal", "every digit value", "every fourth without a value")}


# ---- one call -----------------------------------------------------------------------------------------------------------------

class Held:
    """A call's tensors on the device: the records, the row list, d_order with its canary, the result and d_order_select, the
    outputs filled with FILL"""

    def __init__(self, dev, col, rows_in, room):
        import torch

        self.d_fields = ttd.to_device(dev, np.ascontiguousarray(col)).view(torch.int64).view(-1, 2) if len(col) else torch.zeros((1, 2), dtype=torch.int64, device=dev.device)
        self.d_rows_in = None if rows_in is None else torch.from_numpy(np.ascontiguousarray(rows_in, dtype=np.uint32).view(np.int32).copy()).to(dev.device)
        if rows_in is not None and len(rows_in) == 0:
            self.d_rows_in = torch.zeros((1,), dtype=torch.int32, device=dev.device)
        self.t_order = torch.empty((room + CANARY,), dtype=torch.int32, device=dev.device)
        self.t_res = torch.empty((48,), dtype=torch.uint8, device=dev.device)
        self.t_sel = torch.empty((48,), dtype=torch.uint8, device=dev.device)
        self.refill()

    def refill(self):
        self.t_order.fill_(FILL32 - 2**32), self.t_res.fill_(FILL), self.t_sel.fill_(FILL)


def device_sort(dev, held, stride, R, N, flags, limit, capacity, sel_code, in_code, mode):
    """One call in one mode on `held` as it is -> (d_order with the canary as uint32, the result's bytes, d_order_select's)"""
    import torch

    t_rows_sel = struct_to_device(dev, tcm.select_result(R, sel_code))
    t_in_sel = None if held.d_rows_in is None else struct_to_device(dev, tcm.select_result(N, in_code))
    dev.set_sort_mode(mode)
    rc = dev.lib.msj_sort_rows_device(dev.ctx, held.d_fields.data_ptr() if stride else None, stride, t_rows_sel.data_ptr(),
                                      None if held.d_rows_in is None else held.d_rows_in.data_ptr(), None if t_in_sel is None else t_in_sel.data_ptr(), flags,
                                      limit, held.t_order.data_ptr(), capacity, held.t_res.data_ptr(), held.t_sel.data_ptr(), dev._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return held.t_order.cpu().numpy().view(np.uint32), held.t_res.cpu().numpy(), held.t_sel.cpu().numpy()


def run_sort(dev, stw, col, R, rows_in=None, N=None, flags=0, limit=0, capacity=None, sel_code=0, in_code=0, where=None, modes=MODES):
    """The device in every mode against the twin over the whole of d_order -> the twin's tsm.Sorted"""
    stride = len(col)
    if rows_in is not None:
        rows_in = np.ascontiguousarray(rows_in, dtype=np.uint32)
        N = len(rows_in) if N is None else N
    if capacity is None:
        capacity = len(rows_in) if rows_in is not None else stride
    want = tsm.twin_sort(stw, col, R, rows_in, N, flags, limit, capacity, sel_code, in_code)
    assert want.rc == 0
    want_res = np.frombuffer(bytes(want.res), dtype=np.uint8)
    want_sel = np.frombuffer(bytes(want.order_sel), dtype=np.uint8)
    held = Held(dev, col, rows_in, len(want.order))
    for mode in modes:
        held.refill()
        order, res, sel = device_sort(dev, held, stride, R, N, flags, limit, capacity, sel_code, in_code, mode)
        got = _lib.MsjSortRowsResult.from_buffer_copy(res.tobytes())
        assert np.array_equal(res, want_res), (where, mode, [(n, getattr(got, n), getattr(want.res, n)) for n, _ in got._fields_])
        assert np.array_equal(sel, want_sel), (where, mode, "d_order_select")
        assert (order[len(want.order):] == FILL32).all(), (where, mode, "the canary")
        bad = np.nonzero(order[:len(want.order)] != want.order)[0]      # every entry, the fill behind K included
        assert bad.size == 0, (where, mode, "entry", int(bad[0]), int(order[bad[0]]), int(want.order[bad[0]]), int(bad.size), int(want.res.n_written))
    return want


# ---- sizes and columns ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_columns(dev, stw, n):
    """Every column at every size: all the rows (without a limit every mode is the full sort: one of them at the largest
    size), and a third of them, where mode 2 is the selection"""
    for name, col in columns_of(n, 100 + n).items():
        flags = (0, DESC)[len(name) % 2]
        want = run_sort(dev, stw, col, n, flags=flags, where=(n, name), modes=MODES if n <= 2 * T + 1 else (0,))
        assert want.res.code == 0 and want.res.n_rows == n and want.res.n_written == n
        want = run_sort(dev, stw, col, n, flags=flags, limit=max(1, n // 3), where=(n, name, "a third"))
        assert want.res.code == 0 and want.res.n_written == min(max(1, n // 3), n)
    if n:
        assert run_sort(dev, stw, columns_of(n, 1)["all equal"], n, where=(n, "stable")).rows() == list(range(n))


@pytest.mark.parametrize("n", [257, 2 * T + 1, S * T + 1])
def test_one_digit_differs(dev, stw, n):
    """A column whose keys differ in exactly one digit, for each of the eleven: ten passes skipped, and the order ends in the
    buffer the one pass wrote; then two digits far apart, and all of them"""
    rng = np.random.default_rng(n)
    for digit in range(11):
        if n > 2 * T + 1 and digit != 1:
            continue
        for limit in (0, n // 2):
            want = run_sort(dev, stw, one_digit_column(n, digit, rng), n, flags=DESC if digit % 2 else 0, limit=limit, where=(n, "digit", digit, limit))
            assert want.res.n_written == (limit or n)
    two = one_digit_column(n, 0, rng)
    two["bits"] = (two["bits"].view(np.int64) * np.where(np.arange(n) % 2, 1, -1)).view(np.uint64)      # the sign: hi's top byte
    run_sort(dev, stw, two, n, limit=n // 5, where=(n, "two digits"))


@pytest.mark.parametrize("n", [2 * T + 1, 5 * T + 77])
def test_limits_at_the_cut(dev, stw, n):
    """Limits on both sides of a wave, a block and N, with at least three blocks of equal keys straddling each cut, with the rows without a
    value reaching into the first K, and the same with values_only"""
    rng = np.random.default_rng(n)
    k = np.arange(n)
    # runs of 4 * B equal keys, shuffled over the rows: a cut falls inside a run that three blocks and more hold parts of
    runs = ints(rng.permutation(k // (4 * B)))
    few_values = ints(rng.integers(0, 50, n))
    few_values["type"][k % 8 != 0] = ord("t")                       # an eighth of the rows has a value
    for limit in sorted({1, 2, 10, 255, 256, 257, n - 1, n, n + 1}):
        for flags in (0, DESC):
            want = run_sort(dev, stw, runs, n, flags=flags, limit=limit, where=(n, "runs", limit, flags))
            assert want.res.n_written == min(limit, n)
        want = run_sort(dev, stw, few_values, n, limit=limit, where=(n, "few values", limit))
        assert want.res.n_written == min(limit, n) and want.res.n_values == (n + 7) // 8
        want = run_sort(dev, stw, few_values, n, flags=VALUES_ONLY, limit=limit, where=(n, "values only", limit))
        assert want.res.n_written == min(limit, want.res.n_values)
    same = ints(np.full(n, -9))
    for limit in (1, 3 * B, n - 1):
        assert run_sort(dev, stw, same, n, flags=DESC, limit=limit, where=(n, "all equal", limit)).rows() == list(range(limit))


def test_rows_in(dev, stw):
    """d_rows_in: a filter's d_kept, a reversed list, a list with repeats and entries at and past R"""
    import torch

    n = 3 * T + 5
    rng = np.random.default_rng(5)
    col = without_values(ints(rng.integers(-300, 300, n)), 5, 2)
    # a filter's own output, on the device
    d_fields = ttd.to_device(dev, col).view(torch.int64).view(1, n, 2)
    t_sel = struct_to_device(dev, tcm.select_result(n))
    preds = dev.compile_predicates([(0, ">", -100)])
    res, _, d_kept, d_kept_select, _ = dev.filter_rows(preds, torch.zeros(16, dtype=torch.uint8, device=dev.device), 16, d_fields, t_sel, capacity=n)
    kept = d_kept[:int(res.n_kept)].cpu().numpy().view(np.uint32)
    preds.close()
    dev._paths.remove(preds)
    assert 300 < len(kept) < n
    for mode in MODES:
        dev.set_sort_mode(mode)
        got, d_order, d_order_select = dev.sort_rows(d_fields[0], t_sel, d_kept, d_kept_select, descending=True, limit=300, capacity=n)
        want = tsm.twin_sort(stw, col, n, kept, flags=DESC, limit=300, capacity=n)
        assert bytes(got) == bytes(want.res) and d_order[:300].cpu().numpy().view(np.uint32).tolist() == want.rows()
        assert d_order_select.cpu().numpy().tobytes() == bytes(want.order_sel)
    run_sort(dev, stw, col, n, rows_in=np.arange(n)[::-1], where="reversed")
    hostile = rng.integers(0, n + 40, 2 * n + 3).astype(np.uint32)
    hostile[::97] = 0xFFFFFFFF
    hostile[1::101] = n
    for flags, limit in ((0, 0), (DESC, 0), (VALUES_ONLY, 0), (0, 700), (DESC | VALUES_ONLY, 2 * T)):
        want = run_sort(dev, stw, col, n, rows_in=hostile, flags=flags, limit=limit, where=("repeats", flags, limit))
        assert want.res.n_out_of_range > 40
    # R below the stride and N below the capacity: what lies behind either is not read as a row
    run_sort(dev, stw, col, n - T, rows_in=hostile, N=T + 3, where="R and N below their rooms")


def test_two_keys(dev, stw):
    """The minor key's order as d_rows_in of the major key's call, both on the device: sorted() with a tuple key"""
    import torch

    n = 2 * T + 9
    rng = np.random.default_rng(11)
    major = without_values(pick(np.arange(n) % 2 == 1, ints(rng.integers(0, 6, n)), doubles(rng.integers(0, 6, n).astype(np.float64))), 9, 4)
    minor = doubles(rng.integers(-40, 40, n) * 0.25)
    t_sel = struct_to_device(dev, tcm.select_result(n))
    d_major, d_minor = (ttd.to_device(dev, c).view(torch.int64).view(n, 2) for c in (major, minor))
    value = lambda col, j: tsm.py_value(col[j])[0]
    want = sorted(range(n), key=lambda j: ((value(major, j) is None, value(major, j) or 0), -value(minor, j)))
    for mode in MODES:
        dev.set_sort_mode(mode)
        _, d_first, d_first_select = dev.sort_rows(d_minor, t_sel, descending=True, sync=False)
        res, d_order, _ = dev.sort_rows(d_major, t_sel, d_first, d_first_select, limit=n if mode else 0)
        assert res.code == 0 and res.n_written == n and d_order.cpu().numpy().view(np.uint32).tolist() == want, mode


def test_codes_and_capacities(dev, stw):
    n = T + 9
    col = without_values(ints(np.arange(n)[::-1].copy()), 4, 1)
    rows_in = np.arange(n, dtype=np.uint32)
    for kw in (dict(sel_code=7), dict(rows_in=rows_in, in_code=9, sel_code=7), dict(rows_in=rows_in, sel_code=5)):
        want = run_sort(dev, stw, col, n, limit=10, where=kw, **kw)
        assert want.res.code in (7, 9, 5) and want.res.n_rows == 0 and (want.order == FILL32).all()
    for R, kw in ((n + 1, {}), (n, dict(rows_in=rows_in, capacity=n - 1)), (1 << 31, {}), (n, dict(rows_in=rows_in, N=n + 3)), (n, dict(rows_in=rows_in, N=1 << 31))):
        want = run_sort(dev, stw, col, R, flags=DESC, limit=5, where=(R, kw), **kw)
        assert want.res.code == MSJ_CAPACITY and want.res.n_written == 0 and (want.order == FILL32).all()
    assert run_sort(dev, stw, col, 0, flags=VALUES_ONLY, where="no rows").res.flags == VALUES_ONLY
    assert run_sort(dev, stw, col, n, rows_in=rows_in, N=0, where="no input rows").res.n_written == 0
    assert run_sort(dev, stw, col, n, capacity=n, where="exactly the room").res.n_written == n


def test_check_order(dev):
    """Each is refused with nothing launched, in the header's order: the outputs keep what was in them"""
    import torch

    n = 8
    d_rows = ttd.to_device(dev, tam.records(list(range(n)) + [0] * 8))
    sel, in_sel = struct_to_device(dev, tcm.select_result(n)), struct_to_device(dev, tcm.select_result(n))
    d_in = torch.arange(2 * n, dtype=torch.int32, device=dev.device)
    full = lambda count, dtype: torch.full((count,), 0x5A if dtype == torch.uint8 else 0x5A5A5A5A, dtype=dtype, device=dev.device)
    order, res, out_sel = full(n + 2, torch.int32), full(48, torch.uint8), full(48, torch.uint8)

    def sort(**kw):
        p = dict(ctx=dev.ctx, rows=d_rows.data_ptr(), stride=n, sel=sel.data_ptr(), rows_in=None, in_sel=None, flags=0, limit=0, order=order.data_ptr(), cap=n,
                 res=res.data_ptr(), out_sel=out_sel.data_ptr())
        p.update(kw)
        return dev.lib.msj_sort_rows_device(p["ctx"], p["rows"], p["stride"], p["sel"], p["rows_in"], p["in_sel"], p["flags"], p["limit"], p["order"], p["cap"],
                                            p["res"], p["out_sel"], dev._stream())

    listed = dict(rows_in=d_in.data_ptr(), in_sel=in_sel.data_ptr())
    for name in ("ctx", "res", "sel"):
        assert sort(**{name: None}) == BAD_ARGUMENT, name
    assert sort(rows_in=d_in.data_ptr()) == BAD_ARGUMENT and sort(in_sel=in_sel.data_ptr()) == BAD_ARGUMENT
    assert sort(rows=None) == BAD_ARGUMENT and sort(order=None) == BAD_ARGUMENT and sort(flags=4) == BAD_ARGUMENT and sort(flags=1 << 31) == BAD_ARGUMENT
    # NULL and the flags win over the size, the size over aliasing and alignment
    assert sort(stride=1 << 40, rows=None) == BAD_ARGUMENT and sort(cap=1 << 40, flags=8) == BAD_ARGUMENT
    assert sort(stride=1 << 40, res=sel.data_ptr()) == MSJ_CAPACITY and sort(cap=1 << 40, rows=d_rows.data_ptr() + 8) == MSJ_CAPACITY
    assert sort(res=sel.data_ptr()) == BAD_ARGUMENT and sort(res=out_sel.data_ptr()) == BAD_ARGUMENT and sort(res=in_sel.data_ptr(), **listed) == BAD_ARGUMENT
    assert sort(out_sel=sel.data_ptr()) == BAD_ARGUMENT and sort(out_sel=in_sel.data_ptr(), **listed) == BAD_ARGUMENT
    assert sort(order=d_in.data_ptr() + 4 * (n - 1), **listed) == BAD_ARGUMENT
    assert sort(rows_in=d_in.data_ptr() + 12, in_sel=in_sel.data_ptr(), order=d_in.data_ptr(), limit=4) == BAD_ARGUMENT
    for name, base, step in (("rows", d_rows, 8), ("order", order, 2), ("sel", sel, 4), ("res", res, 4), ("out_sel", out_sel, 4)):
        assert sort(**{name: base.data_ptr() + step}) == BAD_ARGUMENT, name
    assert sort(rows_in=d_in.data_ptr() + 2, in_sel=in_sel.data_ptr()) == BAD_ARGUMENT and sort(rows_in=d_in.data_ptr(), in_sel=in_sel.data_ptr() + 4) == BAD_ARGUMENT
    torch.cuda.synchronize()
    assert bool((order == 0x5A5A5A5A).all()) and bool((res == 0x5A).all()) and bool((out_sel == 0x5A).all()) and d_in.tolist() == list(range(2 * n))
    # what is allowed: the order behind the list, in front of it with a limit that ends before it, no d_order_select, no room
    assert sort(rows_in=d_in.data_ptr() + 12, in_sel=in_sel.data_ptr(), order=d_in.data_ptr(), limit=3, flags=DESC) == 0
    torch.cuda.synchronize()
    assert d_in.tolist() == [7, 6, 5] + list(range(3, 2 * n))      # the rows 3 .. 10 of which 8, 9, 10 have no value: descending 7, 6, 5
    assert sort(order=d_in.data_ptr() + 4 * n, **listed) == 0
    torch.cuda.synchronize()
    assert d_in.tolist() == [7, 6, 5, 3, 4, 5, 6, 7] + [3, 4, 5, 5, 6, 6, 7, 7]
    out_sel.fill_(0x5A)
    assert sort(out_sel=None, limit=2) == 0
    torch.cuda.synchronize()
    assert order.tolist()[:3] == [0, 1, 0x5A5A5A5A] and bool((out_sel == 0x5A).all())
    assert sort(stride=0, rows=None, cap=0, order=None) == 0      # no room for a row: the count alone is MSJ_CAPACITY
    torch.cuda.synchronize()
    got = _lib.MsjSortRowsResult.from_buffer_copy(res.cpu().numpy().tobytes())
    assert got.code == MSJ_CAPACITY and got.n_rows == n and got.n_written == 0
    hook = dev.lib.msj_debug_set_sort_mode
    assert hook(dev.ctx, 3) == BAD_ARGUMENT and hook(None, 0) == BAD_ARGUMENT and hook(dev.ctx, 0) == 0
    ws = dev.lib.msj_sort_rows_workspace_bytes
    assert ws(0) >= 64 and ws(1 << 20) >= ws(0) + 32 * (1 << 20) and ws(1 << 40) == ws(1 << 31)


# ---- end to end -------------------------------------------------------------------------------------------------------------

def log_lines(n):
    lines, docs = [], []
    t0 = datetime.datetime(2024, 5, 1, 12, 0, 0, tzinfo=datetime.timezone.utc)
    for k in range(n):
        when = t0 + datetime.timedelta(microseconds=((k * 7919) % 1000) * 1500 + (k % 3))
        d = {"id": k, "ts": when.strftime("%Y-%m-%dT%H:%M:%S.%f") + "Z", "status": ["ok", "error", "retry"][k % 3],
             "latency_ms": [k * 3 % 101, (k % 50) * 0.5, 9007199254740993 - (k % 4), 9007199254740992.0, -0.0, 2**62 + k % 5][k % 6]}
        if k % 13 == 5:
            d["latency_ms"] = ["slow", None, True][k // 13 % 3]
        if k % 17 == 2:
            del d["latency_ms"]
        if k % 19 == 7:
            d["ts"] = "yesterday"
        lines.append(json.dumps(d).encode()), docs.append(d)
    return lines, docs


def number_of(v):
    from fractions import Fraction

    return Fraction(v) if isinstance(v, (int, float)) and not isinstance(v, bool) else None


def test_window_order_by(dev):
    """Window.order_by over a few hundred NDJSON lines -- the slowest lines, time order by a cast timestamp, two keys, behind a
    filter -- against json.loads and sorted(), then the lines themselves through raw("", compact=True)"""
    import torch
    from mojo_simdjson_amd.document_stream import DocumentStream

    lines, docs = log_lines(500)
    data = b"\n".join(lines) + b"\n"
    seen = windows = 0
    micros = lambda d: datetime.datetime.strptime(d["ts"], "%Y-%m-%dT%H:%M:%S.%fZ") if d["ts"] != "yesterday" else None
    for win in DocumentStream(dev, tvd.upload(dev, data), len(data), window=16384, select=["", "/latency_ms", "/ts", "/status", "/id"]):
        n = win.n_documents
        mine = docs[seen:seen + n]
        lat = [number_of(d.get("latency_ms")) for d in mine]
        slowest = sorted(range(n), key=lambda j: (lat[j] is None, -(lat[j] or 0)))
        top = win.order_by("/latency_ms", descending=True, limit=10)
        assert top.keep is None and top.rows.tolist() == slowest[:10] and top.n_rows == 10
        off, text, ok = top.raw("", compact=True)
        off, text = off.cpu().numpy(), text.cpu().numpy().tobytes()
        assert bool(ok.all()) and [json.loads(text[off[i]:off[i + 1]]) for i in range(10)] == [mine[j] for j in slowest[:10]]
        assert top.values("/id") == [mine[j]["id"] for j in slowest[:10]]
        # every line, the ones without a latency last in their own order; and only the ones with one
        assert win.order_by("/latency_ms", descending=True).rows.tolist() == slowest
        assert win.order_by("/latency_ms", values_only=True).rows.tolist() == sorted((j for j in range(n) if lat[j] is not None), key=lambda j: lat[j])
        # time order: the strings cast to nanoseconds on the device
        when = [micros(d) for d in mine]
        in_time = sorted(range(n), key=lambda j: (when[j] is None, when[j] or datetime.datetime.min))
        by_time = win.order_by("/ts", cast={"/ts": ("timestamp", "ns")})
        assert by_time.rows.tolist() == in_time and by_time.values("/id") == [mine[j]["id"] for j in in_time]
        # two keys: time inside latency, the latency descending
        both = win.order_by([("/latency_ms", "desc"), "/ts"], cast={"/ts": ("timestamp", "us")}, limit=40)
        assert both.rows.tolist() == sorted(range(n), key=lambda j: (lat[j] is None, -(lat[j] or 0), when[j] is None, when[j] or datetime.datetime.min))[:40]
        # behind a filter: the selection's rows are the window's document numbers
        errors = win.where([("/status", "==", "error")])
        kept = [j for j in range(n) if mine[j]["status"] == "error"]
        got = errors.order_by("/latency_ms", limit=7)
        assert got.rows.tolist() == sorted(kept, key=lambda j: (lat[j] is None, lat[j] or 0))[:7] and got.values("/id") == [mine[j]["id"] for j in got.rows.tolist()]
        order, d_order_select = errors.order("/latency_ms", limit=7)
        assert [kept[i] for i in order.tolist()] == got.rows.tolist() and int(d_order_select[8:16].view(torch.int64).item()) == 7
        seen += n
        windows += 1
    assert windows >= 2 and seen == len(docs)
    with pytest.raises(ValueError):
        win.order_by("/latency_ms", limit=0)
    with pytest.raises(ValueError):
        win.order_by(("/latency_ms", "down"))
