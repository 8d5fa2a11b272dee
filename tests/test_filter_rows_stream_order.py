"""msj_filter_rows_device and msj_take_rows_device in stream order (the manner of tests/test_stream_order.py, whose corpus and
helpers are imported as they are): on a side stream, behind inputs that arrive late, with sync=False, every capacity given
and every output a tensor of the caller's.

The decoy window B -- A's sizes, other values -- lies in the window's bytes and in the records, and has been through both
calls: every tensor and both workspaces hold B's consistent state.  Then, on a side stream: a delay, device-to-device copies
of A's bytes and records over them, the outputs back to their fill, and the two calls.  A launch or a memset that dropped its
stream argument runs ahead of the copies and reads the decoy; what it writes is then overwritten with the fill or differs
from A's expected arrays, which come from the host twin (tests/filter_rows_math_host.cpp) alone.
"""
import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from tests import stream_order as so
from tests import test_filter_rows_math as tfm
from tests import test_stream_order as tso
from tests import test_tape_documents as ttd
from tests import test_validate_documents as tvd

SPECS = [tfm.Spec(so.P_STATUS, tfm.STR_EQ, b"active"), tfm.Spec(so.P_STATUS, tfm.STR_PREFIX, b"clo"),
         tfm.Spec(so.P_ITEMS, tfm.TYPE, 2, neg=True)]
DEVICE_SPECS = [(so.P_STATUS, "==", "active"), (so.P_STATUS, "prefix", "clo"), ("not", (so.P_ITEMS, "type", "array"))]


class Expected:
    """Filter (ANY of SPECS) and take over the select twin's records of one window of tests/stream_order.py, on the host"""

    def __init__(self, x):
        ftwin = tfm.load_twin()
        self.x, self.n_paths, self.rows = x, len(so.POINTERS), x.rows
        self.fields = np.ascontiguousarray(x.sel.fields).view(np.uint8).reshape(-1)
        records = np.ascontiguousarray(x.sel.fields).reshape(-1)[:self.n_paths * x.rows]
        blob = tfm.compile_specs(ftwin, SPECS, True)
        self.filtered = tfm.twin_filter(ftwin, blob, x.data, x.length, records, x.rows, self.n_paths, x.sel.res, x.rows)
        f = self.filtered
        assert f.rc == 0 and f.res.code == 0 and 0 < f.res.n_kept < x.D
        self.taken, self.out, self.out_select = tfm.twin_take(ftwin, f.kept[:x.rows], f.kept_select, records, x.rows, self.n_paths, x.sel.res,
                                                              x.rows, x.rows)
        assert self.taken.code == 0 and self.taken.n_rows == f.res.n_kept

    def arrays(self):
        """{name: (the expected bytes, fill and canary included)}"""
        f = self.filtered
        struct = lambda s: np.frombuffer(bytes(s), dtype=np.uint8)
        return {"keep": f.keep, "kept": f.kept.view(np.uint8), "res": struct(f.res), "ksel": struct(f.kept_select),
                "out": self.out.view(np.uint8).reshape(-1), "tres": struct(self.taken), "osel": struct(self.out_select)}


def test_expected_on_cpu():
    """A's and the decoy's expected arrays differ in every output of both calls: a call that read the decoy shows"""
    a, b = Expected(so.expected("A")), Expected(so.expected("B"))
    assert a.x.rows == b.x.rows and a.fields.size == b.fields.size
    for name, want in a.arrays().items():
        other = b.arrays()[name]
        assert want.size == other.size and (name in ("res", "ksel", "tres", "osel") or not np.array_equal(want, other)), name
    assert not np.array_equal(a.arrays()["res"], b.arrays()["res"])


@pytest.mark.gpu
def test_filter_and_take_behind_late_inputs(dev):
    import time

    import torch

    a, b = Expected(so.expected("A")), Expected(so.expected("B"))
    x, rows, n_paths = a.x, a.rows, a.n_paths
    want = a.arrays()
    predicates = dev.compile_predicates(DEVICE_SPECS, any=True)
    d_buf, d_buf_a = tvd.upload(dev, b.x.data), tvd.upload(dev, x.data)
    d_rec, d_rec_a = ttd.to_device(dev, b.fields), ttd.to_device(dev, a.fields)
    d_sel = ttd.to_device(dev, np.frombuffer(bytes(x.sel.res), dtype=np.uint8))   # (the same for both windows: D)
    assert bytes(x.sel.res) == bytes(b.x.sel.res)
    out = {name: ttd.to_device(dev, np.full(w.size, tfm.FILL, dtype=np.uint8)) for name, w in want.items()}
    pristine = {name: t.clone() for name, t in out.items()}
    d_fields = d_rec.view(torch.int64)[:n_paths * rows * 2].view(n_paths, rows, 2)

    def enqueue():
        for name, t in out.items():
            t.copy_(pristine[name], non_blocking=True)
        dev.filter_rows(predicates, d_buf, x.length, d_fields, d_sel, capacity=rows, d_keep=out["keep"], d_kept=out["kept"].view(torch.int32),
                        d_result=out["res"], d_kept_select=out["ksel"], sync=False)
        dev.take_rows(out["kept"].view(torch.int32), out["ksel"], d_fields, d_sel,
                      d_out=out["out"].view(torch.int64)[:n_paths * rows * 2].view(n_paths, rows, 2), out_capacity=rows, d_result=out["tres"],
                      d_out_select=out["osel"], sync=False)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    enqueue()   # the decoy through both calls: the workspaces have their sizes and hold its state
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    for name, w in b.arrays().items():
        assert np.array_equal(out[name].cpu().numpy(), w), ("the decoy", name)
    s = torch.cuda.Stream(dev.device)
    need_ms = max(tso.MIN_DELAY_MS, tso.JITTER * t_enq * 1e3)
    start, ready = tso.delayed(s, need_ms), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        d_buf.copy_(d_buf_a, non_blocking=True)
        d_rec.copy_(d_rec_a, non_blocking=True)
        ready.record()
        enqueue()
    pending = not ready.query()
    s.synchronize()
    delay_ms = start.elapsed_time(ready)
    numbers = f"the enqueue took {t_enq * 1e3:.2f} ms on the host, the delay {delay_ms:.1f} ms of the {need_ms:.1f} ms it has to last"
    print(numbers)
    assert pending, "inconclusive: the inputs were there when the enqueue returned -- a host wait in the calls, or the delay too short: " + numbers
    assert delay_ms >= need_ms, numbers
    for name, w in want.items():
        got = out[name].cpu().numpy()
        bad = np.nonzero(got != w)[0]
        assert bad.size == 0, (name, int(bad[0]), got[bad[:4]].tolist(), w[bad[:4]].tolist(), int(bad.size))
    assert _lib.MsjFilterRowsResult.from_buffer_copy(out["res"].cpu().numpy().tobytes()).n_kept == a.filtered.res.n_kept


@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    d = Stage1Device(0)
    yield d
    d.close()
