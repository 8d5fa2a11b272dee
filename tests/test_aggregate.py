"""Count, sum, min, max per group on the device (msj_aggregate_device, csrc/aggregate_kernel.hip).

Expected values come from the host twin of the same arithmetic (tests/aggregate_math_host.cpp, the minimum and the maximum
by the merge rule row after row), which tests/test_aggregate_math.py holds against the definition written in Python.  Device
output is compared with the twin over the WHOLE record tensor (both start from the fill 0xA5, with room and a canary behind
G, so a store the twin does not make shows) and over the 48-byte result.  Records are made on the host and uploaded; the
end-to-end test runs the real chain through DocumentStream.  Every comparison runs twice, with the switch between the two
paths at 8 groups (msj_debug_set_aggregate_limits) and with the LDS path off: the two have to write the same bytes.

The kernel's constants (csrc/aggregate_kernel.hip) are named below as the shapes use them.
"""
import json
import random
from fractions import Fraction

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from mojo_simdjson_amd.document_stream import FIELD_DTYPE
from tests import test_aggregate_math as tam
from tests import test_string_column_math as tcm
from tests import test_tape_documents as ttd
from tests import test_validate_documents as tvd

pytestmark = pytest.mark.gpu

B = 256          # kRows: rows per workgroup, one per lane
WAVE = 64
LIMIT = 8        # the most groups of the LDS path in these tests
CANARY = 96      # bytes behind the records' capacity
MSJ_CAPACITY, BAD_ARGUMENT = 1, -1
FILL = tam.FILL


@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    d = Stage1Device(0)
    yield d
    d.set_aggregate_limits()
    d.close()


@pytest.fixture(scope="module")
def atw():
    return tam.load_twin()


def struct_to_device(dev, s):
    import torch

    return torch.from_numpy(np.frombuffer(bytes(s), dtype=np.uint8).copy()).to(dev.device)


class Held:
    """A call's tensors on the device -- the records, the codes, d_n_groups, the record tensor with its canary and the result,
    the two outputs filled with FILL -- for a caller that keeps them from one call to the next"""

    def __init__(self, dev, columns, codes, capacity):
        import torch

        columns = tam.as_columns(columns)
        n_columns, stride = columns.shape
        self.d_fields = ttd.to_device(dev, columns.reshape(-1)).view(torch.int64).view(n_columns, stride, 2)
        self.d_codes = None if codes is None else torch.from_numpy(np.ascontiguousarray(codes, dtype=np.int32)).to(dev.device)
        self.t_groups = torch.empty((n_columns * capacity * 48 + CANARY,), dtype=torch.uint8, device=dev.device)
        self.t_res = torch.empty((48,), dtype=torch.uint8, device=dev.device)
        self.d_n = torch.zeros((1,), dtype=torch.int64, device=dev.device)
        self.refill()

    def refill(self):
        self.t_groups.fill_(FILL), self.t_res.fill_(FILL)

    def write_rows(self, columns, codes):
        """The first rows of every column and their codes; what lies behind them stays"""
        import torch

        columns = tam.as_columns(columns)
        n = columns.shape[1]
        self.d_fields[:, :n].copy_(torch.from_numpy(columns.view(np.int64).reshape(columns.shape[0], n, 2).copy()))
        self.d_codes[:n].copy_(torch.from_numpy(np.ascontiguousarray(codes[:n], dtype=np.int32)))


def device_aggregate(dev, columns, R, codes, G, capacity, sel_code=0, by_pointer=False, limit=LIMIT, held=None):
    """One call on hand-made records -> (the record tensor's bytes with the canary, the result's bytes).  held: the call runs
    on these tensors as they are, whatever an earlier call left in them, and not on an upload of `columns` and `codes`"""
    import torch

    h = Held(dev, columns, codes, capacity) if held is None else held
    t_sel = struct_to_device(dev, tcm.select_result(R, sel_code))
    if by_pointer:
        h.d_n.fill_(G)
    dev.set_aggregate_limits(limit)
    res, _ = dev.aggregate(h.d_fields, t_sel, h.d_codes, n_groups=0x7777 if by_pointer else G, d_n_groups=h.d_n if by_pointer else None,
                           d_groups=h.t_groups, groups_capacity=capacity, d_result=h.t_res, sync=False)
    assert res is h.t_res
    torch.cuda.synchronize()
    return h.t_groups.cpu().numpy(), h.t_res.cpu().numpy()


def run_aggregate(dev, atw, columns, R, codes, G, capacity=None, sel_code=0, by_pointer=False, where=None, limits=(LIMIT, 0), held=None):
    """The device, with the switch at LIMIT groups and with the LDS path off, against the twin over the whole of the record
    tensor -> the twin's tam.Agg.  held: a Held of these columns and codes, uploaded once for all the limits; its outputs
    are filled again before every call"""
    capacity = G + 2 if capacity is None else capacity
    want = tam.twin_aggregate(atw, columns, R, codes, G, capacity=capacity, sel_code=sel_code)
    assert want.rc == 0
    want_res = np.frombuffer(bytes(want.res), dtype=np.uint8)
    for limit in limits:
        if held is not None:
            held.refill()
        groups, res = device_aggregate(dev, columns, R, codes, G, capacity, sel_code, by_pointer, limit, held)
        assert (groups[len(want.groups):] == FILL).all(), (where, limit, "the canary")
        got = _lib.MsjAggregateResult.from_buffer_copy(res.tobytes())
        assert np.array_equal(res, want_res), (where, limit, [(n, getattr(got, n), getattr(want.res, n)) for n, _ in got._fields_])
        bad = np.nonzero(groups[:len(want.groups)] != want.groups)[0]
        if bad.size:
            i = int(bad[0]) // 48
            raise AssertionError((where, limit, "record", i, groups[48 * i:48 * i + 48].view(tam.AGG_DTYPE), want.groups[48 * i:48 * i + 48].view(tam.AGG_DTYPE),
                                  int(bad.size)))
    return want


def make_rows(seed, R, G, n_columns=1, stride=None):
    """n_columns columns of R mixed records (one zero record behind them) and a code per row: most in [0, G), some -1, G and
    INT32_MIN; every group has its own centre of exponents"""
    rng = random.Random(seed)
    stride = R + 1 if stride is None else stride
    centres = [rng.randrange(0, 2047) for _ in range(max(G, 1))]
    ints_only = [rng.random() < 0.25 for _ in range(max(G, 1))]
    codes = np.zeros(stride, dtype=np.int32)
    columns = np.zeros((n_columns, stride), dtype=FIELD_DTYPE)
    for k in range(R):
        g = rng.choice([-1, G, -(2**31)]) if rng.random() < 0.08 or G == 0 else rng.randrange(G)
        if G and rng.random() < 0.3:      # runs of one group: whole waves of it
            g = (k // 100) % G
        codes[k] = g
        for c in range(n_columns):
            v = tam.random_value(rng, centres[g if 0 <= g < G else 0])
            if 0 <= g < G and ints_only[g] and not isinstance(v, (int, tam.Raw)):
                v = int(v) if abs(v) < 2**62 else tam.INT64_MAX
            columns[c, k] = tam.record(v)
    return columns, codes


# ---- sizes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [0, 1, 63, 64, 65, 255, 256, 257, 4097])
def test_rows_and_groups(dev, atw, R):
    """Every row count against every group count on both sides of the switch"""
    for G in sorted({1, 2, 37, LIMIT - 1, LIMIT, LIMIT + 1, R}):
        columns, codes = make_rows(1000 * R + G, R, G)
        want = run_aggregate(dev, atw, columns, R, codes, G, where=(R, G))
        assert want.res.code == 0 and want.res.n_rows == R and want.res.n_groups == G and (R < 64 or G == 0 or want.res.n_values > 0)


@pytest.mark.parametrize("n_columns", [1, 3])
def test_columns(dev, atw, n_columns):
    """Three columns with a stride above the rows: column c's records at c * groups_capacity"""
    R = 2 * B + 37
    for G in (LIMIT, 37):
        columns, codes = make_rows(77 + G, R, G, n_columns, stride=R + 11)
        want = run_aggregate(dev, atw, columns, R, codes, G, capacity=G + 5, where=(n_columns, G))
        per_column = want.records(G)["n_values"].sum(axis=1)
        assert want.res.code == 0 and (per_column > 0).all() and want.res.n_values == per_column.sum()
        assert n_columns == 1 or len({bytes(want.records(G)[c].tobytes()) for c in range(n_columns)}) == n_columns


# ---- the pinned cases ---------------------------------------------------------------------------------------------------------

def test_pinned_cases_at_block_edges(dev, atw):
    """Every case of tests/test_aggregate_math.py as a group of its own, its values in the first and the last row of
    successive blocks; the rows between belong to one more group or to none"""
    names = sorted(tam.CASES)
    G = len(names) + 1
    slots = []
    for i, name in enumerate(names):
        for j, v in enumerate(tam.CASES[name]):
            slots.append((i, v))
    R = B * ((len(slots) + 1) // 2)
    values = [(1.5 if k % 3 else k) for k in range(R)]
    codes = np.array([G - 1 if k % 5 else -1 for k in range(R)] + [0], dtype=np.int32)
    for s, (i, v) in enumerate(slots):
        k = (s // 2) * B + (B - 1 if s % 2 else 0)
        values[k], codes[k] = v, i
    columns = tam.records(values + [0])
    for G_call in (G, LIMIT):      # all the cases past the switch, and the first eight below it
        want = run_aggregate(dev, atw, columns, R, codes, G_call, where="pinned")
        got = want.records(G_call)[0]
        for i, name in enumerate(names[:G_call]):
            expect, _ = tam.py_group([tam.record(v) for v in tam.CASES[name]])
            assert tuple(int(x) for x in got[i]) == expect, name


# ---- the arguments' forms -------------------------------------------------------------------------------------------------------

def test_no_codes(dev, atw):
    """d_codes == NULL: every row is group 0, whatever G says; every wave is of one group"""
    R = 3 * B + 5
    columns, _ = make_rows(31, R, 1, 2)
    for G in (1, 3, LIMIT + 1, 0):
        want = run_aggregate(dev, atw, columns, R, None, G, where=("no codes", G))
        assert want.res.n_ungrouped == (R if G == 0 else 0) and (G == 0 or want.records(G)[0, 0]["n_rows"] == R)
        assert G < 2 or not want.records(G)[:, 1:].view(np.uint8).any()


def test_groups_by_pointer(dev, atw):
    """G read on the device gives what G by value gives (n_groups is then not looked at)"""
    R = B + 77
    for G in (5, LIMIT + 3):
        columns, codes = make_rows(9 + G, R, G)
        by_value = run_aggregate(dev, atw, columns, R, codes, G, capacity=G + 3, where=("by value", G))
        by_pointer = run_aggregate(dev, atw, columns, R, codes, G, capacity=G + 3, by_pointer=True, where=("by pointer", G))
        assert np.array_equal(by_value.groups, by_pointer.groups)


def test_capacities_and_codes(dev, atw):
    R, G = B + 9, 12
    columns, codes = make_rows(5, R, G)
    want = run_aggregate(dev, atw, columns, R, codes, G, capacity=G - 1, where="one group short")
    assert want.res.code == MSJ_CAPACITY and want.res.n_groups == G and want.res.n_rows == R and (want.groups == FILL).all()
    want = run_aggregate(dev, atw, columns, R + 2, codes, G, where="rows over the stride")
    assert want.res.code == MSJ_CAPACITY and want.res.n_rows == R + 2 and (want.groups == FILL).all()
    want = run_aggregate(dev, atw, columns, 1 << 31, codes, G, where="2^31 rows")
    assert want.res.code == MSJ_CAPACITY and want.res.n_rows == 1 << 31
    want = run_aggregate(dev, atw, columns, R, codes, G, sel_code=5, where="a code")
    assert want.res.code == 5 and want.res.n_rows == 0 and (want.groups == FILL).all()
    want = run_aggregate(dev, atw, columns, R, codes, G, capacity=G, where="exactly the room")
    assert want.res.code == 0
    want = run_aggregate(dev, atw, columns, R, codes, 0, capacity=0, where="no room, no groups")
    assert want.res.code == 0 and want.res.n_ungrouped == R


# ---- the same bytes, whatever the order -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [3, 37, 900])
def test_same_bytes_for_every_order(dev, atw, G):
    """The same input twice and once with rows and codes permuted together, on each path: identical bytes five times"""
    R = 4 * B + 19
    columns, codes = make_rows(404 + G, R, G, 2, stride=R)
    first = run_aggregate(dev, atw, columns, R, codes, G, capacity=G, where=("first", G))
    seen = [device_aggregate(dev, columns, R, codes, G, G, limit=limit) for limit in (LIMIT, 0, _lib.AGG_MAX_LDS_GROUPS)]
    perm = np.random.default_rng(G).permutation(R)
    seen += [device_aggregate(dev, columns[:, perm], R, codes[perm], G, G, limit=limit) for limit in (LIMIT, 0, _lib.AGG_MAX_LDS_GROUPS)]
    want_res = np.frombuffer(bytes(first.res), dtype=np.uint8)
    for groups, res in seen:
        assert np.array_equal(groups[:len(first.groups)], first.groups) and np.array_equal(res, want_res)


# ---- the order of the argument checks -----------------------------------------------------------------------------------------

def test_check_order(dev):
    """Each is refused with nothing launched, in the header's order: the outputs keep what was in them"""
    import torch

    R, G = 8, 2
    d_rows = ttd.to_device(dev, tam.records(list(range(R)) + [0] * 8))
    d_codes = torch.tensor([0, 1] * 8, dtype=torch.int32, device=dev.device)
    sel = struct_to_device(dev, tcm.select_result(R))
    full = lambda n: torch.full((n,), 0x5A, dtype=torch.uint8, device=dev.device)
    out, res, d_n = full(48 * (G + 2)), full(48), torch.tensor([G, 0], dtype=torch.int64, device=dev.device)

    def agg(**kw):
        p = dict(ctx=dev.ctx, rows=d_rows.data_ptr(), stride=R, cols=1, sel=sel.data_ptr(), codes=d_codes.data_ptr(), G=G, d_n=None,
                 out=out.data_ptr(), cap=G, res=res.data_ptr())
        p.update(kw)
        return dev.lib.msj_aggregate_device(p["ctx"], p["rows"], p["stride"], p["cols"], p["sel"], p["codes"], p["G"], p["d_n"], p["out"], p["cap"],
                                            p["res"], dev._stream())

    for name in ("ctx", "res", "sel", "rows", "out"):
        assert agg(**{name: None}) == BAD_ARGUMENT, name
    assert agg(cols=0) == BAD_ARGUMENT and agg(cols=17) == BAD_ARGUMENT
    # NULL and the column count win over the size, the size over aliasing and alignment
    assert agg(stride=1 << 40, out=None) == BAD_ARGUMENT and agg(cap=1 << 40, cols=0) == BAD_ARGUMENT
    assert agg(stride=1 << 40, res=sel.data_ptr()) == MSJ_CAPACITY and agg(cap=1 << 40, rows=d_rows.data_ptr() + 8) == MSJ_CAPACITY
    assert agg(res=sel.data_ptr()) == BAD_ARGUMENT
    for name, base, step in (("rows", d_rows, 8), ("out", out, 8), ("codes", d_codes, 2), ("d_n", d_n, 4), ("sel", sel, 4), ("res", res, 4)):
        assert agg(**{name: base.data_ptr() + step}) == BAD_ARGUMENT, name
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all()) and bool((res == 0x5A).all())
    assert agg(stride=0, rows=None) == 0       # no room for a row: the count alone is MSJ_CAPACITY
    torch.cuda.synchronize()
    assert _lib.MsjAggregateResult.from_buffer_copy(res.cpu().numpy().tobytes()).code == MSJ_CAPACITY and bool((out == 0x5A).all())
    assert agg(cap=0, out=None, G=0) == 0 and agg(codes=None, d_n=d_n.data_ptr()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[48 * G:] == 0x5A).all() and got[:48 * G].view(tam.AGG_DTYPE)["n_rows"].tolist() == [R, 0]
    assert got[:48].view(tam.AGG_DTYPE)["sum_bits"][0] == sum(range(R))
    hook = dev.lib.msj_debug_set_aggregate_limits
    assert hook(dev.ctx, _lib.AGG_MAX_LDS_GROUPS + 1) == BAD_ARGUMENT and hook(None, 0) == BAD_ARGUMENT and hook(dev.ctx, _lib.AGG_MAX_LDS_GROUPS) == 0
    ws = dev.lib.msj_aggregate_workspace_bytes
    assert ws(0, 0, 1) >= 64 and ws(1 << 20, 1000, 3) >= ws(0, 0, 1) + 3 * 1000 * 96 and ws(1 << 30, 5, 1) == ws(0, 5, 1)


# ---- end to end -------------------------------------------------------------------------------------------------------------

STATUSES = ["ok", "error", "timeout", "ok", "ok", "retry", "error", "ok"]


def log_lines(n):
    lines, docs = [], []
    for k in range(n):
        d = {"status": STATUSES[(k * 7) % len(STATUSES)], "latency_ms": [k * 3 + 1, (k % 50) * 0.1, 9007199254740993 - k, -0.0, 1e300, 2**62][k % 6],
             "items": [{"qty": (k + j) % 7, "price": 0.25 * j} for j in range(k % 4)]}
        if k % 13 == 5:
            d["latency_ms"] = ["slow", None, True][k // 13 % 3]
        if k % 17 == 2:
            del d["latency_ms"]
        if k % 29 == 3:
            d["status"] = 7
        lines.append(json.dumps(d).encode()), docs.append(d)
    return lines, docs


def py_stats(values):
    """What to_python gives for one group's json.loads values, by the yardstick of tests/test_aggregate_math.py"""
    recs = [tam.record(v) if isinstance(v, (int, float)) and not isinstance(v, bool) else tam.Raw(0, "n").t for v in values]
    (n_rows, n_values, sum_bits, min_bits, max_bits, st, lt, ht, flags, _), _ = tam.py_group(recs)
    number = lambda t, b: None if t == 0 else (b - (1 << 64) if b >> 63 else b) if t == tam.L else tam.bits_double(b)
    return {"n_rows": n_rows, "n_values": n_values, "sum": number(st, sum_bits), "min": number(lt, min_bits), "max": number(ht, max_bits), "flags": flags}


def same_stats(got, want):
    """Equal as Python values, the type and the sign of a zero included"""
    key = lambda d: {k: (type(v).__name__, repr(v)) for k, v in d.items() if k != "key"}
    return key(got) == key(want)


def test_window_stats(dev):
    """Window.stats(["/latency_ms"], by="/status") and where(...).stats(...) over a few hundred NDJSON lines, the per-document
    sums of a list column's elements, and the ungrouped form, against json.loads and Fraction"""
    from mojo_simdjson_amd.document_stream import DocumentStream

    lines, docs = log_lines(400)
    data = b"\n".join(lines) + b"\n"
    seen = windows = 0
    for win in DocumentStream(dev, tvd.upload(dev, data), len(data), window=16384, select=["/status", "/latency_ms", "/items"]):
        D = win.n_documents
        mine = docs[seen:seen + D]
        stats = win.stats(["/latency_ms"], by="/status")
        got = stats.to_python()
        keys = [d["status"] for d in mine if isinstance(d["status"], str)]
        order = list(dict.fromkeys(keys))      # a dictionary numbers its values by first appearance
        assert [g["key"] for g in got] == order and stats.keys is not None
        for g in got:
            want = py_stats([d.get("latency_ms", None) for d in mine if d["status"] == g["key"]])
            assert same_stats(g["/latency_ms"], want), (windows, g, want)
        assert stats.n_ungrouped == sum(not isinstance(d["status"], str) for d in mine)
        # the whole window as one group
        total = win.stats(["/latency_ms"]).to_python()
        assert len(total) == 1 and "key" not in total[0] and same_stats(total[0]["/latency_ms"], py_stats([d.get("latency_ms") for d in mine]))
        # behind a filter
        sel = win.where([("/latency_ms", ">", 100)])
        kept = [d for d in mine if isinstance(d.get("latency_ms"), (int, float)) and not isinstance(d.get("latency_ms"), bool) and d["latency_ms"] > 100]
        got = sel.stats(["/latency_ms"], by="/status").to_python()
        assert [g["key"] for g in got] == list(dict.fromkeys(d["status"] for d in kept if isinstance(d["status"], str)))
        for g in got:
            assert same_stats(g["/latency_ms"], py_stats([d["latency_ms"] for d in kept if d["status"] == g["key"]])), (windows, g)
        # sum(items[*].qty) per document
        fields = win.elements("/items").select(["/qty", "/price"])
        per_row = fields.stats(["/qty", "/price"], per_row=True).to_python()
        assert len(per_row) == D
        for d, g in zip(mine, per_row):
            assert same_stats(g["/qty"], py_stats([x["qty"] for x in d["items"]])) and same_stats(g["/price"], py_stats([x["price"] for x in d["items"]]))
        seen += D
        windows += 1
    assert windows >= 2 and seen == len(docs)
    assert Fraction(9007199254740993) != Fraction(float(9007199254740993))     # what a cast to double would have lost
