"""Rows by predicate on the device (msj_filter_rows_device, msj_take_rows_device, csrc/filter_rows_kernel.hip).

Expected values come from the host twin of the same arithmetic (tests/filter_rows_math_host.cpp), which
tests/test_filter_rows_math.py holds against a yardstick written in Python.  Device output is compared with the twin over the
WHOLE d_keep, d_kept, d_list_offsets_out and d_out arrays (both start from the same fill, with 64 bytes of canary behind each
capacity, so a store the twin does not make shows) and over the results and the select results.  Records are generated on
the host and uploaded; the end-to-end test runs the real chain through DocumentStream.

The kernels' constants (csrc/filter_rows_kernel.hip) are named below as the shapes use them.
"""
import ctypes
import json

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from mojo_simdjson_amd.document_stream import FIELD_DTYPE
from tests import test_filter_rows_math as tfm
from tests import test_string_column_math as tcm
from tests import test_tape_documents as ttd
from tests import test_validate_documents as tvd

pytestmark = pytest.mark.gpu

B = 256                  # kRows: rows per workgroup, one per lane
ROW_GRID = 4096 * B      # kGridBlocks = 4096 blocks of kRows rows, `v += gridDim.x`
SCAN_CHUNK = 1024        # wave_ops.h, scan_in_place: blocks of rows per chunk of the running sum
WAVE = 64
MSJ_CAPACITY, BAD_ARGUMENT = 1, -1
Spec = tfm.Spec


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
def ftwin():
    return tfm.load_twin()


def struct_to_device(dev, s):
    import torch

    return torch.from_numpy(np.frombuffer(bytes(s), dtype=np.uint8).copy()).to(dev.device)


def device_predicates(dev, specs, any_=False):
    """msj_predicates_create over the same msj_predicate structs the twin compiles"""
    table, alive = tfm.spec_table(specs)
    h = ctypes.c_void_p()
    assert dev.lib.msj_predicates_create(dev.ctx, table, len(specs), tfm.ANY if any_ else 0, ctypes.byref(h)) == 0
    return h


class Rows:
    """Records on the host and on the device: FIELD_DTYPE[n_columns * stride], the window's bytes"""

    def __init__(self, dev, fields, stride, n_columns, data=b""):
        import torch

        self.fields, self.stride, self.n_columns, self.data = np.ascontiguousarray(fields), stride, n_columns, data
        padded = np.concatenate([self.fields, np.zeros(1, dtype=FIELD_DTYPE)])
        self.d_fields = ttd.to_device(dev, padded)
        self.d_buf = torch.from_numpy(np.frombuffer(data + b"\0" * 16, dtype=np.uint8).copy()).to(dev.device)


def run_filter(dev, ftwin, a, specs, R, capacity=None, any_=False, mask_only=False, list_offsets=None, list_rows=None, list_n_rows=None,
               sel_code=0, where=None):
    """The device against the twin over the whole of every array -> the twin's tfm.Filtered"""
    import torch

    capacity = a.stride if capacity is None else capacity
    sel = tcm.select_result(R, sel_code)
    if list_offsets is not None:
        list_offsets = np.ascontiguousarray(list_offsets, dtype=np.uint64)
        list_rows = list_offsets.size - 1 if list_rows is None else list_rows
    want = tfm.twin_filter(ftwin, tfm.compile_specs(ftwin, specs, any_), a.data, len(a.data), a.fields, a.stride, a.n_columns, sel, capacity,
                           mask_only, list_offsets, list_rows, list_n_rows)
    assert want.rc == 0
    keep, kept, list_out = tfm.filled_filter(capacity, mask_only, list_rows if list_offsets is not None else None)
    up = lambda x: torch.from_numpy(x).to(dev.device)
    t_keep = up(keep)
    t_kept = up(kept.view(np.int32)) if kept is not None else None
    t_list_out = up(list_out.view(np.int64)) if list_out is not None else None
    t_list = ttd.to_device(dev, list_offsets) if list_offsets is not None else None
    t_n = ttd.to_device(dev, np.array([list_n_rows], dtype=np.uint64)) if list_n_rows is not None else None
    t_res = torch.full((48,), tfm.FILL, dtype=torch.uint8, device=dev.device)
    t_ksel = torch.full((48,), tfm.FILL, dtype=torch.uint8, device=dev.device)
    h = device_predicates(dev, specs, any_)
    t_sel = struct_to_device(dev, sel)
    try:
        rc = dev.lib.msj_filter_rows_device(dev.ctx, h, a.d_buf.data_ptr(), len(a.data), a.d_fields.data_ptr(), a.stride, a.n_columns,
                                            t_sel.data_ptr(), t_keep.data_ptr(), t_kept.data_ptr() if t_kept is not None else None,
                                            capacity, t_list.data_ptr() if t_list is not None else None, list_rows or 0,
                                            t_n.data_ptr() if t_n is not None else None, t_list_out.data_ptr() if t_list_out is not None else None,
                                            t_res.data_ptr(), t_ksel.data_ptr(), dev._stream())
        assert rc == 0, (where, rc)
        torch.cuda.synchronize()
    finally:
        dev.lib.msj_predicates_destroy(h)
    res = _lib.MsjFilterRowsResult.from_buffer_copy(t_res.cpu().numpy().tobytes())
    ksel = _lib.MsjSelectDocumentsResult.from_buffer_copy(t_ksel.cpu().numpy().tobytes())
    got = tfm.Filtered(rc, res, t_keep.cpu().numpy(), t_kept.cpu().numpy().view(np.uint32) if t_kept is not None else None,
                       t_list_out.cpu().numpy().view(np.uint64) if t_list_out is not None else None, ksel)
    assert got.summary() == want.summary(), (where, got.summary(), want.summary())
    assert got.select_summary() == want.select_summary(), (where, got.select_summary(), want.select_summary())
    for name in ("keep", "kept", "list_out"):
        x, y = getattr(got, name), getattr(want, name)
        if y is None:
            assert x is None
            continue
        bad = np.nonzero(x != y)[0]
        assert bad.size == 0, (where, name, int(bad[0]), x[bad[:4]].tolist(), y[bad[:4]].tolist(), bad.size)
    return want


def run_take(dev, ftwin, a, take, K, R, out_capacity=None, out_stride=None, take_code=0, sel_code=0, where=None):
    """The device's take against the twin's over the whole output array -> (the twin's result, its records)"""
    import torch

    take = np.ascontiguousarray(take, dtype=np.uint32)
    out_capacity = K if out_capacity is None else out_capacity
    out_stride = out_capacity if out_stride is None else out_stride
    take_sel, rows_sel = tcm.select_result(K, take_code), tcm.select_result(R, sel_code)
    want, want_out, want_sel = tfm.twin_take(ftwin, take, take_sel, a.fields, a.stride, a.n_columns, rows_sel, out_stride, out_capacity)
    t_take = ttd.to_device(dev, np.concatenate([take, np.zeros(4, dtype=np.uint32)]))
    t_out = torch.full((want_out.size * 2 + 2,), 0, dtype=torch.int64, device=dev.device)
    t_out[:] = int(np.full(8, tfm.FILL, dtype=np.uint8).view(np.int64)[0])
    t_res = torch.full((48,), tfm.FILL, dtype=torch.uint8, device=dev.device)
    t_osel = torch.full((48,), tfm.FILL, dtype=torch.uint8, device=dev.device)
    t_take_sel, t_rows_sel = struct_to_device(dev, take_sel), struct_to_device(dev, rows_sel)
    rc = dev.lib.msj_take_rows_device(dev.ctx, t_take.data_ptr(), t_take_sel.data_ptr(), a.d_fields.data_ptr(), a.stride,
                                      a.n_columns, t_rows_sel.data_ptr(), t_out.data_ptr(), out_stride, out_capacity,
                                      t_res.data_ptr(), t_osel.data_ptr(), dev._stream())
    assert rc == 0, (where, rc)
    torch.cuda.synchronize()
    res = _lib.MsjTakeRowsResult.from_buffer_copy(t_res.cpu().numpy().tobytes())
    osel = _lib.MsjSelectDocumentsResult.from_buffer_copy(t_osel.cpu().numpy().tobytes())
    assert tfm.take_summary(res) == tfm.take_summary(want), (where, tfm.take_summary(res), tfm.take_summary(want))
    s = lambda x: (x.code, x.flags, x.n_documents, x.n_paths, x.n_found, x.n_no_bits, x.reserved)
    assert s(osel) == s(want_sel), (where, s(osel), s(want_sel))
    got_out = t_out.cpu().numpy().view(np.uint8)[:want_out.size * 16]
    bad = np.nonzero(got_out != want_out.view(np.uint8))[0]
    assert bad.size == 0, (where, int(bad[0]) // 16, bad.size)
    assert bool((t_out.cpu().numpy().view(np.uint8)[want_out.size * 16:] == tfm.FILL).all())
    return want, want_out


def int_records(values):
    """'l' records of the values, generated"""
    f = np.zeros(len(values), dtype=FIELD_DTYPE)
    f["bits"], f["token"], f["type"] = np.asarray(values, dtype=np.int64).view(np.uint64), np.arange(len(values), dtype=np.uint32), ord("l")
    return f


def mixed_records(rng, n, data_len):
    """Records of every kind tfm.all_kinds knows, drawn"""
    pool = np.concatenate(tfm.all_kinds(data_len))
    return pool[rng.integers(pool.size, size=n)]


MIXED_DATA = b'"A"  \\u0041B'
MIXED_SPECS = [Spec(0, tfm.TYPE, 4 | 8 | 16), Spec(1, tfm.NUM_GT, 250.25, neg=True), Spec(2, tfm.STR_PREFIX, b"A")]


# ---- row counts and the grid --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, B - 1, B, B + 1])
def test_row_counts(dev, ftwin, n):
    """No row, one row, and the block border, over three columns of records of every kind: ALL and ANY, with list offsets
    over the rows, and the take of the kept rows"""
    rng = np.random.default_rng(n)
    a = Rows(dev, mixed_records(rng, 3 * n, len(MIXED_DATA)), n, 3, MIXED_DATA)
    offs = np.sort(rng.integers(0, n + 1, 12)).astype(np.uint64)
    for any_ in (False, True):
        want = run_filter(dev, ftwin, a, MIXED_SPECS, n, any_=any_, list_offsets=offs, where=(n, any_))
        K = int(want.res.n_kept)
        assert want.list_out[11] == int(want.keep[:int(offs[11])].sum()) and K == int(want.keep[:n].sum())
        run_take(dev, ftwin, a, want.kept[:K], K, n, where=(n, any_))
    assert n < 2 or 0 < K < n


@pytest.mark.parametrize("n", [SCAN_CHUNK * B + 1, ROW_GRID + 1])
def test_past_the_scan_chunk_and_the_row_grid(dev, ftwin, n):
    """One row past a chunk of the scan over the block counts (262 145 rows), and one past the row grid (1 048 577): every
    third row and the last one kept"""
    values = (np.arange(n, dtype=np.int64) % 3 == 0).astype(np.int64)
    values[n - 1] = 1
    a = Rows(dev, int_records(values), n, 1)
    offs = np.array([0, 1, n - 1, n, n + 5, B, SCAN_CHUNK * B, 7], dtype=np.uint64)
    want = run_filter(dev, ftwin, a, [Spec(0, tfm.NUM_EQ, 1)], n, list_offsets=offs, where=n)
    K = int(want.res.n_kept)
    assert K == int(values.sum()) and want.kept[K - 1] == n - 1 and want.keep[:n].tolist() == values.tolist()
    take = np.concatenate([want.kept[:K:2], [n - 1, n, 0xFFFFFFFF, 0]]).astype(np.uint32)
    got, out = run_take(dev, ftwin, a, take, take.size, n, where=n)
    assert got.n_out_of_range == 2 and out["token"][:4].tolist() == want.kept[:8:2].tolist()


def keep_pattern(name, R):
    k = np.arange(R)
    return {"none": k < 0, "all": k >= 0, "every other": k % 2 == 1, "only row 0": k == 0, "only the last row": k == R - 1,
            "the last lane of each wave": k % WAVE == WAVE - 1, "a full block next to an empty one": (k // B) % 2 == 0}[name].astype(np.int64)


@pytest.mark.parametrize("name", ["none", "all", "every other", "only row 0", "only the last row", "the last lane of each wave",
                                  "a full block next to an empty one"])
def test_keep_patterns(dev, ftwin, name):
    R = 4 * B + 17
    values = keep_pattern(name, R)
    a = Rows(dev, int_records(values), R, 1)
    want = run_filter(dev, ftwin, a, [Spec(0, tfm.NUM_GE, 0.5)], R, where=name)
    assert want.keep[:R].tolist() == values.tolist() and want.kept[:int(want.res.n_kept)].tolist() == np.nonzero(values)[0].tolist()
    run_filter(dev, ftwin, a, [Spec(0, tfm.NUM_GE, 0.5)], R, mask_only=True, where=name)


@pytest.mark.parametrize("n_columns", [1, 16])
def test_columns(dev, ftwin, n_columns):
    """One column and sixteen, a predicate on the last one, sixteen predicates, a stride above the capacity"""
    rng = np.random.default_rng(n_columns)
    R, stride = 2 * B + 3, 2 * B + 9
    a = Rows(dev, mixed_records(rng, n_columns * stride, len(MIXED_DATA)), stride, n_columns, MIXED_DATA)
    last = n_columns - 1
    run_filter(dev, ftwin, a, [Spec(last, tfm.FOUND)], R, capacity=R, where=n_columns)
    pool = tfm.every_spec()
    specs = [Spec(int(rng.integers(n_columns)), s.op, s.operand, s.neg) for s in (pool[int(j)] for j in rng.integers(len(pool), size=16))]
    specs[3].column = last
    for any_ in (False, True):
        want = run_filter(dev, ftwin, a, specs, R, capacity=R, any_=any_, where=(n_columns, any_))
        K = int(want.res.n_kept)
        run_take(dev, ftwin, a, want.kept[:K], K, R, out_stride=K + 5, where=n_columns)


def test_strings_across_a_block_border(dev, ftwin):
    """STR_EQ and STR_PREFIX on a window whose escaped values straddle the block border: the value "error" plain, with one
    escape, wholly escaped, a longer value, a shorter one, no string, a span past the window"""
    forms = [b"error", b"err\\u006fr", b"\\u0065\\u0072\\u0072\\u006f\\u0072", b"errors", b"erro", b"\\u20acrror", b"warn\\n", b""]
    data, records = bytearray(), []
    R = 2 * B + 11
    for k in range(R):
        body = forms[(k * 5 + k // B) % len(forms)]
        data += b'{"s":"'
        records.append(tfm.string_rec(len(data), len(body), b"\\" in body))
        data += body + b'"}\n'
    fields = np.concatenate(records)
    fields[B - 2] = tfm.int_rec(5)[0]
    fields[B + 1] = tfm.error_rec(20)[0]
    fields[R - 1] = tfm.string_rec(len(data) - 2, 3)[0]
    a = Rows(dev, fields, R, 1, bytes(data))
    for specs in ([Spec(0, tfm.STR_EQ, b"error")], [Spec(0, tfm.STR_PREFIX, b"err")], [Spec(0, tfm.STR_PREFIX, b"\xe2\x82")],
                  [Spec(0, tfm.STR_EQ, b"error", neg=True), Spec(0, tfm.STR_PREFIX, b"")], [Spec(0, tfm.STR_EQ, b"")]):
        want = run_filter(dev, ftwin, a, specs, R, where=specs[0].operand)
        assert 0 < want.res.n_kept < R
    want = run_filter(dev, ftwin, a, [Spec(0, tfm.STR_EQ, b"error")], R)
    assert want.keep[:8].tolist() == [int(forms[(k * 5) % 8] in forms[:3]) for k in range(8)]


# ---- capacities ---------------------------------------------------------------------------------------------------------------

def test_capacities(dev, ftwin):
    """capacity = R - 1 and out_capacity = K - 1: MSJ_CAPACITY and nothing else written; a code in the select result; R read
    from the device word while the host's capacity is larger; a stride below R in the take"""
    R = B + 40
    values = keep_pattern("every other", R)
    a = Rows(dev, int_records(values), R, 1)
    spec = [Spec(0, tfm.NUM_EQ, 1)]
    over = run_filter(dev, ftwin, a, spec, R, capacity=R - 1)
    assert over.summary() == (MSJ_CAPACITY, 0, R, 0, 0, 0, 0)
    coded = run_filter(dev, ftwin, a, spec, R, sel_code=7)
    assert coded.summary() == (7, 0, 0, 0, 0, 0, 0)
    small = run_filter(dev, ftwin, a, spec, 70, capacity=R)   # the device word decides
    assert small.res.n_rows == 70 and small.res.n_kept == 35
    want = run_filter(dev, ftwin, a, spec, R)
    K = int(want.res.n_kept)
    short, _ = run_take(dev, ftwin, a, want.kept[:K], K, R, out_capacity=K - 1)
    assert tfm.take_summary(short) == (MSJ_CAPACITY, 0, K, 0, 0, 0, 0)
    assert run_take(dev, ftwin, a, want.kept[:K], K, R + 1)[0].code == MSJ_CAPACITY      # more rows than a column has room for
    assert run_take(dev, ftwin, a, want.kept[:K], K, R, take_code=9)[0].code == 9
    assert run_take(dev, ftwin, a, want.kept[:K], K, R, sel_code=4)[0].code == 4
    fewer, out = run_take(dev, ftwin, a, want.kept[:K], 10, R, out_capacity=K)            # K from the device word
    assert fewer.n_rows == 10 and fewer.n_found == 10


def test_list_rebasing(dev, ftwin):
    """Offsets of a list column over the rows: empty lists, a list whose elements all go, P past a block, P from the device
    word, offsets that descend or exceed R, and a P above the caller's arrays"""
    rng = np.random.default_rng(5)
    P = B + 10
    lengths = rng.integers(0, 6, P)
    lengths[::7] = 0
    gone = 3 * (P // 4) + 1
    lengths[gone] = 4
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    R = int(offs[-1])
    values = rng.integers(0, 3, R).astype(np.int64)
    values[int(offs[gone]):int(offs[gone + 1])] = 0
    a = Rows(dev, int_records(values), R, 1)
    spec = [Spec(0, tfm.NUM_GT, 0)]
    want = run_filter(dev, ftwin, a, spec, R, list_offsets=offs)
    new = want.list_out[:P + 1].tolist()
    assert new[0] == 0 and new[-1] == want.res.n_kept and new[gone] == new[gone + 1]
    assert [new[r + 1] - new[r] for r in range(P)] == [int((values[int(offs[r]):int(offs[r + 1])] > 0).sum()) for r in range(P)]
    run_filter(dev, ftwin, a, spec, R, list_offsets=offs, list_n_rows=B - 1)
    over = run_filter(dev, ftwin, a, spec, R, list_offsets=offs, list_n_rows=P + 1)
    assert over.res.code == MSJ_CAPACITY and over.res.n_kept == want.res.n_kept
    bad = offs.copy()
    bad[5], bad[40], bad[B + 2], bad[9] = R + 3, 0xFFFFFFFFFFFFFFFF, 1, 0
    run_filter(dev, ftwin, a, spec, R, list_offsets=bad)
    run_filter(dev, ftwin, a, spec, 0, list_offsets=bad)


def test_hostile_records(dev, ftwin):
    """Records of every kind over more than a block, 200 of them with bits from a generator -- spans anywhere, any int64, any
    double -- and a take by a vector of any numbers"""
    rng = np.random.default_rng(99)
    R = 3 * B + 5
    fields = mixed_records(rng, 2 * R, len(MIXED_DATA))
    hostile = rng.integers(0, 2 * R, 200)
    fields["bits"][hostile] = rng.integers(0, 1 << 63, 200, dtype=np.uint64) * 2 + 1
    a = Rows(dev, fields, R, 2, MIXED_DATA)
    specs = [Spec(0, tfm.STR_PREFIX, b"A"), Spec(1, tfm.STR_EQ, b"AB"), Spec(1, tfm.NUM_LT, 1e300), Spec(0, tfm.NUM_GE, -2**63)]
    want = run_filter(dev, ftwin, a, specs, R, any_=True)
    assert 0 < want.res.n_kept < R
    take = rng.integers(0, 2 * R, 500).astype(np.uint32)
    take[::50] = 0xFFFFFFFF
    got, _ = run_take(dev, ftwin, a, take, take.size, R, out_stride=520)
    assert got.n_out_of_range > 0 and got.n_found > 0


# ---- the order of the argument checks ------------------------------------------------------------------------------------------

def test_check_order(dev):
    """Each is refused with nothing launched, in the header's order: the outputs keep what was in them"""
    import torch

    R = 8
    a = Rows(dev, int_records(np.arange(R)), R, 1)
    h1 = device_predicates(dev, [Spec(0, tfm.NUM_GT, 3)])
    h2 = device_predicates(dev, [Spec(1, tfm.FOUND)])
    sel = struct_to_device(dev, tcm.select_result(R))
    full = lambda n, dtype: torch.full((n * torch.empty(0, dtype=dtype).element_size(),), 0x5A, dtype=torch.uint8, device=dev.device).view(dtype)
    keep, kept, res, ksel = full(16, torch.uint8), full(16, torch.int32), full(48, torch.uint8), full(48, torch.uint8)
    offs, offs_out, n_rows = torch.zeros(4, dtype=torch.int64, device=dev.device), full(4, torch.int64), torch.full((2,), 3, dtype=torch.int64, device=dev.device)
    out, tres, osel = full(2 * 16, torch.int64), full(48, torch.uint8), full(48, torch.uint8)

    def filt(**kw):
        p = dict(ctx=dev.ctx, preds=h1, buf=a.d_buf.data_ptr(), len=0, fields=a.d_fields.data_ptr(), stride=R, cols=1, sel=sel.data_ptr(),
                 keep=keep.data_ptr(), kept=kept.data_ptr(), cap=R, offs=offs.data_ptr(), list_rows=3, n_rows=n_rows.data_ptr(),
                 offs_out=offs_out.data_ptr(), res=res.data_ptr(), ksel=ksel.data_ptr())
        p.update(kw)
        return dev.lib.msj_filter_rows_device(p["ctx"], p["preds"], p["buf"], p["len"], p["fields"], p["stride"], p["cols"], p["sel"], p["keep"],
                                              p["kept"], p["cap"], p["offs"], p["list_rows"], p["n_rows"], p["offs_out"], p["res"], p["ksel"],
                                              dev._stream())

    for name in ("ctx", "preds", "res", "sel", "buf", "fields", "keep", "offs", "offs_out"):
        assert filt(**{name: None}) == BAD_ARGUMENT, name
    assert filt(cols=0) == BAD_ARGUMENT and filt(cols=17) == BAD_ARGUMENT and filt(preds=h2) == BAD_ARGUMENT
    assert filt(cols=2, stride=R - 1) == BAD_ARGUMENT
    # NULL wins over the size, the size over aliasing and alignment
    assert filt(len=(1 << 32) + 1, keep=None) == BAD_ARGUMENT
    assert filt(len=(1 << 32) + 1, fields=a.d_fields.data_ptr() + 8) == MSJ_CAPACITY
    assert filt(res=sel.data_ptr()) == BAD_ARGUMENT and filt(ksel=sel.data_ptr()) == BAD_ARGUMENT and filt(ksel=res.data_ptr()) == BAD_ARGUMENT
    for name, base, step in (("fields", a.d_fields, 8), ("kept", kept, 2), ("offs", offs, 4), ("offs_out", offs_out, 4), ("n_rows", n_rows, 4),
                             ("sel", sel, 4), ("res", res, 4), ("ksel", ksel, 4)):
        assert filt(**{name: base.data_ptr() + step}) == BAD_ARGUMENT, name

    tsel = struct_to_device(dev, tcm.select_result(4))
    take = torch.tensor([7, 0, 9, 7, 0, 0, 0, 0], dtype=torch.int32, device=dev.device)

    def tk(**kw):
        p = dict(ctx=dev.ctx, take=take.data_ptr(), tsel=tsel.data_ptr(), fields=a.d_fields.data_ptr(), stride=R, cols=1, sel=sel.data_ptr(),
                 out=out.data_ptr(), out_stride=4, cap=4, res=tres.data_ptr(), osel=osel.data_ptr())
        p.update(kw)
        return dev.lib.msj_take_rows_device(p["ctx"], p["take"], p["tsel"], p["fields"], p["stride"], p["cols"], p["sel"], p["out"],
                                            p["out_stride"], p["cap"], p["res"], p["osel"], dev._stream())

    for name in ("ctx", "res", "tsel", "sel", "take", "out", "fields"):
        assert tk(**{name: None}) == BAD_ARGUMENT, name
    assert tk(cols=0) == BAD_ARGUMENT and tk(cols=17) == BAD_ARGUMENT and tk(cols=2, out_stride=3) == BAD_ARGUMENT
    assert tk(out=a.d_fields.data_ptr()) == BAD_ARGUMENT and tk(out=a.d_fields.data_ptr() + 16 * (R - 1)) == BAD_ARGUMENT
    assert tk(fields=out.data_ptr() + 16 * 3) == BAD_ARGUMENT
    assert tk(res=tsel.data_ptr()) == BAD_ARGUMENT and tk(res=sel.data_ptr()) == BAD_ARGUMENT and tk(osel=tsel.data_ptr()) == BAD_ARGUMENT
    assert tk(osel=sel.data_ptr()) == BAD_ARGUMENT and tk(osel=tres.data_ptr()) == BAD_ARGUMENT
    for name, base, step in (("fields", a.d_fields, 8), ("out", out, 8), ("take", take, 2), ("tsel", tsel, 4), ("sel", sel, 4), ("res", tres, 4),
                             ("osel", osel, 4)):
        assert tk(**{name: base.data_ptr() + step}) == BAD_ARGUMENT, name
    torch.cuda.synchronize()
    for t in (keep, res, ksel, tres, osel):
        assert bool((t == 0x5A).all())
    assert bool((kept == 0x5A5A5A5A).all()) and bool((offs_out == 0x5A5A5A5A5A5A5A5A).all()) and bool((out == 0x5A5A5A5A5A5A5A5A).all())
    # create: NULL, the counts, a column above 15, an operand over 255 bytes, an unknown op and flag -- and then the calls run
    hh = ctypes.c_void_p()
    table, alive = tfm.spec_table([Spec(0, tfm.FOUND)] * 17)
    create = dev.lib.msj_predicates_create
    assert create(None, table, 1, 0, ctypes.byref(hh)) == BAD_ARGUMENT and create(dev.ctx, table, 1, 0, None) == BAD_ARGUMENT
    assert create(dev.ctx, None, 1, 0, ctypes.byref(hh)) == BAD_ARGUMENT
    assert create(dev.ctx, table, 0, 0, ctypes.byref(hh)) == BAD_ARGUMENT and create(dev.ctx, table, 17, 0, ctypes.byref(hh)) == BAD_ARGUMENT
    assert create(dev.ctx, table, 1, 2, ctypes.byref(hh)) == BAD_ARGUMENT
    for bad in (Spec(16, tfm.FOUND), Spec(0, 9), Spec(0, tfm.STR_EQ, b"x" * 256), Spec(0, tfm.NUM_EQ, float("inf")), Spec(0, tfm.TYPE, 0),
                Spec(0, tfm.TYPE, 256)):
        one, alive = tfm.spec_table([bad])
        assert create(dev.ctx, one, 1, 0, ctypes.byref(hh)) == BAD_ARGUMENT
    flagged = _lib.MsjPredicate(0, tfm.FOUND, 4, 0, 0, None)
    assert create(dev.ctx, ctypes.byref(flagged), 1, 0, ctypes.byref(hh)) == BAD_ARGUMENT and not hh.value
    dev.lib.msj_predicates_destroy(None)
    assert filt() == 0 and tk() == 0
    torch.cuda.synchronize()
    assert keep.cpu().tolist()[:R + 1] == [0, 0, 0, 0, 1, 1, 1, 1, 0x5A] and kept.cpu().tolist()[:5] == [4, 5, 6, 7, 0x5A5A5A5A]
    assert offs_out.cpu().tolist() == [0, 0, 0, 0]
    assert out.cpu().numpy().view(FIELD_DTYPE)["bits"][:5].tolist() == [7, 0, 0, 7, 0x5A5A5A5A5A5A5A5A]
    assert out.cpu().numpy().view(FIELD_DTYPE)["code"][:4].tolist() == [0, 0, 20, 0]
    ws = dev.lib.msj_filter_rows_workspace_bytes
    assert ws(0) >= 64 and ws(1 << 20) >= ws(0) + 4 * (1 << 20) + 8 * (1 << 12)
    dev.lib.msj_predicates_destroy(h1)
    dev.lib.msj_predicates_destroy(h2)


# ---- end to end -------------------------------------------------------------------------------------------------------------

LATENCIES = [100, 250, 251, 250.5, 250.75, 2**53, 2**53 + 1, float(2**53), 9007199254740993, -1, 1e300, "slow", None, 9007199254740992.5e0, 300]


def log_lines(n):
    """n generated NDJSON lines -> (lines, the documents as json.loads gives them or None for one with a verdict code, each
    document's minified text)"""
    status = ["error", "ok", "warn", "errör", "error", "erro"]
    lines, docs, mini = [], [], []
    for k in range(n):
        d = {"status": status[(k * k + k // 7) % 6], "latency": LATENCIES[(k * 7 + k // 11) % len(LATENCIES)],
             "tags": ["t%d" % (k % 4), "t1%d" % (k % 3), k][:k % 4], "attrs": {"host": "h%d" % (k % 5), "n%d" % (k % 3): k},
             "items": [{"sku": "s%d" % j, "qty": (j + k) % 4 if j != 2 else 1.5} for j in range(k % 5)]}
        if d["latency"] is None:
            del d["latency"]
        if k % 17 == 3:
            del d["status"]
        if k % 19 == 4:
            d["status"] = 5
        if k % 23 == 5:
            d["tags"], d["attrs"] = "none", [1, 2]
        if k % 29 == 6:
            d["items"] = {"qty": 3}
        text = json.dumps(d, indent=None if k % 2 else 1, ensure_ascii=False).encode()
        small = json.dumps(d, separators=(",", ":"), ensure_ascii=False).encode()
        if k % 31 == 11:   # the value written with an escape: the same string
            text = small = small.replace(b'"status":"error"', b'"status":"err\\u006fr"')
        if k == 47:        # a document with a verdict code, whose fields would pass
            text, d, small = b'{"status":"error","latency":300,"tags":[tru]}', None, None
        lines.append(text), docs.append(d), mini.append(small)
    return lines, docs, mini


def test_document_stream_where(dev):
    """DocumentStream(select=[...]) over about 2 000 generated lines in several windows: Window.where against the same
    filter in Python over json.loads -- rows, values, strings, number_column; raw("", compact=True) against the minified
    text of exactly the kept lines; elements and entries of the selection; the where of a list column and of the fields of
    its elements, offsets included; Window.take by the first rows of the distinct statuses."""
    import torch
    from mojo_simdjson_amd.document_stream import DocumentStream, RowSelection

    lines, docs, mini = log_lines(2000)
    data = b"\n".join(lines) + b"\n"
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
    passes = lambda d: d is not None and d.get("status") == "error" and number(d.get("latency")) and d["latency"] > 250.5

    def rows_of(column, n):
        offsets, out, valid = column
        assert offsets.is_cuda and out.is_cuda and offsets.shape == (n + 1,) and valid.shape == (n,)
        off, text, ok = offsets.cpu().tolist(), out.cpu().numpy().tobytes(), valid.cpu().tolist()
        return [text[off[k]:off[k + 1]] if ok[k] else None for k in range(n)]

    seen = windows = kept_in_all = 0
    for win in DocumentStream(dev, tvd.upload(dev, data), len(data), window=65536, select=["", "/status", "/latency", "/tags", "/attrs", "/items"]):
        D = win.n_documents
        mine, small = docs[seen:seen + D], mini[seen:seen + D]
        sel = win.where([("/status", "==", "error"), ("/latency", ">", 250.5)])
        want = [k for k in range(D) if passes(mine[k])]
        kept = [mine[k] for k in want]
        assert isinstance(sel, RowSelection) and sel.rows.is_cuda and sel.rows.dtype == torch.int32 and sel.fields.shape == (6, len(want), 2)
        assert sel.rows.cpu().tolist() == want and sel.n_rows == len(want), windows
        assert sel.keep.cpu().tolist() == [k in set(want) for k in range(D)]
        assert sel.values("/status") == ["error"] * len(want) and sel.values("/latency") == [d["latency"] for d in kept]
        assert rows_of(sel.strings("/status"), len(want)) == [b"error"] * len(want)
        values, valid = sel.number_column("/latency")
        assert valid.cpu().tolist() == [True] * len(want) and values.cpu().tolist() == [float(d["latency"]) for d in kept]
        assert rows_of(sel.raw("", compact=True), len(want)) == [small[k] for k in want], windows
        assert sel.elements("/tags").to_python() == [d["tags"] if isinstance(d["tags"], list) else None for d in kept]
        assert sel.entries("/attrs").to_python() == [d["attrs"] if isinstance(d["attrs"], dict) else None for d in kept]
        # ("not", spec) passes a document without the value; any=True
        either = win.where([("not", ("/status", "found")), ("/latency", "==", 2**53 + 1)], any=True)
        assert either.rows.cpu().tolist() == [k for k in range(D) if mine[k] is None or "status" not in mine[k] or
                                              (number(mine[k].get("latency")) and mine[k]["latency"] == 2**53 + 1)]
        # items[*].qty > 1 stays a list column
        items = win.elements("/items")
        lists = [d["items"] if d is not None and isinstance(d["items"], list) else None for d in mine]
        big = items.select(["/qty", "/sku"]).where([("/qty", ">", 1)])
        left = [[x for x in row if x["qty"] > 1] if row is not None else None for row in lists]
        assert big.values("/qty") == [x["qty"] for row in left if row for x in row] and big.n_elements == big.list_column.n_elements
        assert big.list_column.to_python() == left and big.list_column.valid.cpu().tolist() == [row is not None for row in lists]
        assert big.list_column.offsets.cpu().tolist() == np.concatenate([[0], np.cumsum([len(row or []) for row in left])]).tolist()
        assert big.to_python() == [[{"/qty": x["qty"], "/sku": x["sku"]} for x in row] if row is not None else None for row in left]
        tags = win.elements("/tags").where([(0, "prefix", "t1")])
        tag_lists = [d["tags"] if d is not None and isinstance(d["tags"], list) else None for d in mine]
        assert tags.to_python() == [[x for x in row if isinstance(x, str) and x.startswith("t1")] if row is not None else None for row in tag_lists]
        # one row per distinct status
        cats = win.categories("/status")
        one_each = win.take(cats.first)
        assert one_each.values("/status") == cats.values() and one_each.keep is None and one_each.n_rows == cats.n_distinct >= 5
        past = win.take(torch.tensor([D, 0, D - 1, 0], dtype=torch.int32))
        assert past.values("") == [None, mine[0], mine[D - 1], mine[0]] and past.column("")["code"].tolist()[0] == 20
        seen += D
        windows += 1
        kept_in_all += len(want)
    assert windows >= 4 and seen == len(docs) and kept_in_all > 40
    assert docs[47] is None and passes(json.loads(lines[47].replace(b"[tru]", b"[]")))
    assert any(passes(d) and b"\\u006f" in t for d, t in zip(docs, lines))


def test_record_views_agree(dev):
    """The same records through different views give the same columns: 300 generated lines (the rows cross one block of 256)
    in windows of 16 KiB (about 95 documents each; the arrays are reused) and again as one window (the rows cross the block).
    Per window: the RowSelection that takes every document in order against
    the Window, method by method; the ElementFields that selects "" -- each element itself -- against its ListColumn; the
    values of a map column as a ListColumn, whose text is what json.dumps makes of the entries' values; and the
    RowSelection that takes no document: columns of length 0, one group without a value, no group when grouped by a path."""
    import torch
    from mojo_simdjson_amd.document_stream import DocumentStream, ListColumn

    lines, docs, _ = log_lines(300)
    data = b"\n".join(lines) + b"\n"
    paths = ["", "/status", "/latency", "/tags", "/attrs", "/items"]
    host = lambda t: t.cpu().tolist()
    pair = lambda c: (host(c[0]), host(c[1]))                                      # values, valid
    column = lambda c: (host(c[0]), c[1].cpu().numpy().tobytes(), host(c[2]))      # offsets, bytes, valid
    coded = lambda c: (host(c.codes), c.values(), host(c.first), host(c.valid))
    per_path = [lambda v, p: v.values(p), lambda v, p: column(v.strings(p)), lambda v, p: column(v.raw(p)),
                lambda v, p: column(v.raw(p, compact=True)), lambda v, p: coded(v.categories(p)), lambda v, p: pair(v.timestamps(p)),
                lambda v, p: pair(v.timestamps(p, unit="s")), lambda v, p: pair(v.parsed_numbers(p)),
                lambda v, p: pair(v.parsed_numbers(p, dtype=torch.int64, keep_numbers=False))]
    d_data = tvd.upload(dev, data)
    stream = lambda window: DocumentStream(dev, d_data, len(data), window=window, select=paths)
    seen = windows = 0
    for win in (w for window in (16384, 1 << 20) for w in stream(window)):   # (lazily: a window's arrays are the next one's)
        D = win.n_documents
        sel = win.take(torch.arange(D, dtype=torch.int32))
        assert sel.n_rows == D and sel.fields.shape == win.d_fields.shape
        for p in paths:
            for f in per_path:
                assert f(sel, p) == f(win, p), (windows, p)
            for dtype in (torch.int64, torch.float64):
                assert pair(sel.number_column(p, dtype)) == pair(win.number_column(p, dtype)), (windows, p)
        grouped = win.stats(["/latency"], by="/status").to_python()
        assert sel.stats(["/latency"], by="/status").to_python() == grouped and len(grouped) >= 5
        assert sel.stats(["/latency", "/status"]).to_python() == win.stats(["/latency", "/status"]).to_python()
        tags, attrs = win.elements("/tags"), win.entries("/attrs")
        assert sel.elements("/tags").to_python() == tags.to_python() and sel.entries("/attrs").to_python() == attrs.to_python()
        assert tags.n_elements > D // 2 and attrs.n_entries > D
        # each element itself as the one field of the elements
        ef = tags.select([""])
        assert ef.n_elements == tags.n_elements and ef.values("") == [x for row in tags.to_python() if row for x in row]
        for dtype in (torch.int64, torch.float64):
            assert pair(ef.numbers("", dtype)) == pair(tags.numbers(dtype))
        assert column(ef.strings("")) == column(tags.strings()) and coded(ef.categories("")) == coded(tags.categories())
        assert column(ef.raw("")) == column(tags.raw()) and column(ef.raw("", compact=True)) == column(tags.raw(compact=True))
        assert pair(ef.timestamps("")) == pair(tags.timestamps()) and pair(ef.parsed_numbers("")) == pair(tags.parsed_numbers())
        assert ef.stats([""]).to_python() == tags.stats().to_python()
        assert ef.stats([""], per_row=True).to_python() == tags.stats(per_row=True).to_python()
        # a map column's values as a list column
        values = attrs.values()
        assert isinstance(values, ListColumn) and values.parent is attrs and values.n_elements == attrs.n_entries
        offsets, text, valid = column(values.raw())
        want = [json.dumps(x, ensure_ascii=False).encode() for row in attrs.to_python() if row is not None for x in row.values()]
        assert [text[offsets[j]:offsets[j + 1]] for j in range(attrs.n_entries)] == want and valid == [True] * len(want)
        mine = docs[seen % len(docs):seen % len(docs) + D]
        assert attrs.to_python() == [d["attrs"] if d is not None and isinstance(d["attrs"], dict) else None for d in mine]
        # no row at all
        empty = win.take(torch.zeros(0, dtype=torch.int32))
        assert empty.n_rows == 0 and empty.fields.shape == (len(paths), 0, 2)
        for p in paths:
            assert empty.values(p) == [] and empty.column(p).shape == (0,)
            for f in per_path[1:4]:
                assert f(empty, p) == ([0], b"", [])
            assert coded(empty.categories(p)) == ([], [], [], [])
            for f in per_path[5:]:
                assert f(empty, p) == ([], [])
            assert pair(empty.number_column(p)) == pair(empty.number_column(p, torch.int64)) == ([], [])
        assert empty.elements("/tags").to_python() == [] and empty.entries("/attrs").to_python() == []
        alone = empty.stats(["/latency"])
        assert alone.n_groups == 1 and host(alone.n_values) == [[0]] and host(alone.n_rows) == [0]
        assert empty.stats(["/latency"], by="/status").to_python() == []
        seen += D
        windows += 1
    assert windows >= 4 and seen == 2 * len(docs) and D == len(docs) > 256
