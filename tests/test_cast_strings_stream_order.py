"""msj_cast_strings_device in stream order (the manner of tests/test_filter_rows_stream_order.py; the delay and its bounds are
tests/test_stream_order.py's, tests/stream_order.py is used as it is for the fill): on a side stream, behind inputs that arrive
late, with sync=False, the capacity given and every output a tensor of the caller's.

The decoy window B -- A's sizes, other digits -- lies in the window's bytes and in the records, and has been through the call:
every tensor and the workspace hold B's consistent state.  Then, on a side stream: a delay, device-to-device copies of A's
bytes and records over them, the outputs back to their fill, and the call.  A launch or a memset that dropped its stream
argument runs ahead of the copies and reads the decoy; what it writes is then overwritten with the fill or differs from A's
expected arrays, which come from the host twin (tests/cast_strings_math_host.cpp) alone.  With nullptr for `stream` at
msj_launch_cast_strings (tried once on a copy of the tree, with the first set-up) the test fails at the array "out", record 0:
the kernels ran on the null stream ahead of the side stream's copies, cast the decoy's bytes, and the side stream's reset of
the outputs then left the fill where A's records belong; "res" and "osel" differ likewise.

The second set-up runs two contexts on two streams in turns, A on one and B on the other, with nothing waited for.
"""
import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from tests import stream_order as so
from tests import test_cast_strings_math as tcs
from tests import test_stream_order as tso
from tests import test_tape_documents as ttd
from tests import test_validate_documents as tvd

ROWS = 2000
CALLS = (("timestamp", "ms", False), ("timestamp", "ns", True), ("number", "ns", True))
KINDS = {"timestamp": tcs.TIMESTAMP, "number": tcs.NUMBER}
_DIGITS = bytes.maketrans(b"123456789", b"234567891")


def bodies(decoy):
    """Timestamps and quoted numbers in turn, every seventh spelled with an escape (the list), every eleventh no member; the
    decoy: the same widths and escapes, other digits"""
    out = []
    for k in range(ROWS):
        v = (b"2024-05-%02dT%02d:%02d:%02d.%03dZ" % (1 + k % 28, k % 24, k % 60, (k * 7) % 60, k % 1000)) if k % 2 else b"%d.%03de-2" % (10**6 + k * 7919, k % 1000)
        if k % 11 == 0:
            v = v[:-1] + b"x"
        if decoy:
            v = v[:3] + v[3:].translate(_DIGITS)
        out.append(tcs.escape_at(v, 3 + k % 5) if k % 7 == 0 else v)
    return out


class Expected:
    """The three calls over one window on the host: a cast out of place, one that keeps numbers, the number kind"""

    def __init__(self, decoy):
        ctw = tcs.load_twin()
        self.data, self.records = tcs.window_of(bodies(decoy))
        self.records[5::13]["type"] = ord("l")      # numbers among the strings: kept, or code 17
        self.rows = len(self.records)
        self.casts = [tcs.twin_cast(ctw, self.data, self.records, KINDS[kind], unit if kind == "timestamp" else "s", tcs.KEEP_NUMBERS if keep else 0)
                      for kind, unit, keep in CALLS]
        assert all(c.rc == 0 and c.res.code == 0 and min(c.res.n_cast, c.res.n_syntax) > 100 for c in self.casts)

    def arrays(self):
        """{name: (the expected bytes, fill and canary included)}"""
        struct = lambda s: np.frombuffer(bytes(s), dtype=np.uint8)
        out = {}
        for j, c in enumerate(self.casts):
            out.update({f"out{j}": c.out, f"res{j}": struct(c.res), f"osel{j}": struct(c.sel)})
        return out


def test_expected_on_cpu():
    """A's and the decoy's expected arrays have the same sizes and differ in the records of every call: a call that read the
    decoy shows"""
    a, b = Expected(False), Expected(True)
    assert a.rows == b.rows and len(a.data) == len(b.data) and so.SENTINEL != tcs.FILL
    for name, want in a.arrays().items():
        other = b.arrays()[name]
        assert want.size == other.size and (not name.startswith("out") or not np.array_equal(want, other)), name


class Tensors:
    """The inputs and the caller's output tensors of the three calls on one device"""

    def __init__(self, dev, x, start):
        import torch

        self.dev, self.x = dev, x
        self.d_buf = tvd.upload(dev, start.data)
        self.d_rec = ttd.to_device(dev, start.records).view(torch.int64).view(-1, 2)
        self.d_sel = ttd.to_device(dev, np.frombuffer(bytes(tcs.tcm.select_result(x.rows)), dtype=np.uint8))
        self.out = {name: ttd.to_device(dev, np.full(w.size, tcs.FILL, dtype=np.uint8)) for name, w in x.arrays().items()}
        self.pristine = {name: t.clone() for name, t in self.out.items()}

    def reset(self):
        for name, t in self.out.items():
            t.copy_(self.pristine[name], non_blocking=True)

    def call(self, j):
        import torch

        kind, unit, keep = CALLS[j]
        rows = self.x.rows
        self.dev.cast_strings(self.d_buf, len(self.x.data), self.d_rec, self.d_sel, kind, unit, keep, capacity=rows,
                              d_out=self.out[f"out{j}"].view(torch.int64)[:2 * rows].view(rows, 2), d_result=self.out[f"res{j}"],
                              d_out_select=self.out[f"osel{j}"], sync=False)

    def check(self, want, where):
        for name, w in want.items():
            got = self.out[name].cpu().numpy()
            bad = np.nonzero(got != w)[0]
            assert bad.size == 0, (where, name, int(bad[0]) // 16, got[bad[:4]].tolist(), w[bad[:4]].tolist(), int(bad.size))


@pytest.mark.gpu
def test_cast_behind_late_inputs(dev):
    import time

    import torch

    a, b = Expected(False), Expected(True)
    t = Tensors(dev, a, b)
    d_buf_a, d_rec_a = tvd.upload(dev, a.data), ttd.to_device(dev, a.records).view(torch.int64).view(-1, 2)

    def enqueue():
        t.reset()
        for j in range(len(CALLS)):
            t.call(j)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    enqueue()   # the decoy through the calls: the workspace has its size and holds its state
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    t.check(b.arrays(), "the decoy")
    s = torch.cuda.Stream(dev.device)
    need_ms = max(tso.MIN_DELAY_MS, tso.JITTER * t_enq * 1e3)
    start, ready = tso.delayed(s, need_ms), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        t.d_buf.copy_(d_buf_a, non_blocking=True)
        t.d_rec.copy_(d_rec_a, non_blocking=True)
        ready.record()
        enqueue()
    pending = not ready.query()
    s.synchronize()
    delay_ms = start.elapsed_time(ready)
    numbers = f"the enqueue took {t_enq * 1e3:.2f} ms on the host, the delay {delay_ms:.1f} ms of the {need_ms:.1f} ms it has to last"
    print(numbers)
    assert pending, "inconclusive: the inputs were there when the enqueue returned -- a host wait in the call, or the delay too short: " + numbers
    assert delay_ms >= need_ms, numbers
    t.check(a.arrays(), "behind late inputs")
    assert _lib.MsjCastStringsResult.from_buffer_copy(t.out["res0"].cpu().numpy().tobytes()).n_cast == a.casts[0].res.n_cast


@pytest.mark.gpu
def test_two_contexts_two_streams():
    """Two contexts on two side streams, A on one and the decoy B on the other, the calls enqueued in turns with nothing
    waited for: device state that the process holds once would be shared by the two"""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    devs = [Stage1Device(0), Stage1Device(0)]
    try:
        windows = [Expected(False), Expected(True)]
        sets = [Tensors(d, x, x) for d, x in zip(devs, windows)]
        for t in sets:   # every workspace has its size
            t.call(0)
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(d.device) for d in devs]
        for s, t in zip(streams, sets):
            with torch.cuda.stream(s):
                t.reset()
        for _ in range(3):
            for j in range(len(CALLS)):
                for s, t in zip(streams, sets):
                    with torch.cuda.stream(s):
                        t.call(j)
        for s in streams:
            s.synchronize()
        for t, x in zip(sets, windows):
            t.check(x.arrays(), "two contexts")
    finally:
        for d in devs:
            d.close()


@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    d = Stage1Device(0)
    yield d
    d.close()
