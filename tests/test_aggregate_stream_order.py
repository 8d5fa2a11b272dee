"""msj_aggregate_device in stream order (the manner of tests/test_cast_strings_stream_order.py; the delay and its bounds are
tests/test_stream_order.py's): on a side stream, behind inputs that arrive late, with sync=False, the capacities given and
every output a tensor of the caller's.

The decoy B -- A's sizes, other values and other codes -- lies in the records and in the codes, and has been through the
call: every tensor and the workspace hold B's consistent state.  Then, on a side stream: a delay, device-to-device copies of
A's records and codes over them, the outputs back to their fill, and the call.  A launch or a memset that dropped its stream
argument runs ahead of the copies and reads the decoy; what it writes is then overwritten with the fill or differs from A's
expected arrays, which come from the host twin (tests/aggregate_math_host.cpp) alone.  With nullptr for `stream` at
msj_launch_aggregate (tried once on a copy of the tree, with the first set-up) the test fails at the array "groups0": the
kernels ran on the null stream ahead of the side stream's copies, and the side stream's reset of the outputs then left the
fill where A's records belong.

The second set-up runs two contexts on two streams in turns, A on one and B on the other, with nothing waited for.
"""
import numpy as np
import pytest

from tests import test_aggregate_math as tam
from tests import test_string_column_math as tcm
from tests import test_stream_order as tso
from tests import test_tape_documents as ttd

ROWS = 3000
CALLS = ((5, 2, True), (700, 2, True), (1, 1, False))     # groups, columns, with codes: the LDS path, the global path, no codes
SENTINEL = 0x5C


class Expected:
    """The three calls over one set of records on the host"""

    def __init__(self, decoy):
        atw = tam.load_twin()
        self.rows = ROWS
        self.columns, self.codes = [], []
        for j, (G, n_columns, _) in enumerate(CALLS):
            values, codes = tam.random_groups(100 + j + (50 if decoy else 0), G, most=2 * ROWS // G)
            values, codes = (values + [0] * ROWS)[:ROWS], np.resize(codes, ROWS)
            cols = np.stack([tam.records(values), tam.records(values[::-1])])[:n_columns]
            self.columns.append(np.ascontiguousarray(cols)), self.codes.append(codes)
        self.aggs = [tam.twin_aggregate(atw, self.columns[j], ROWS, self.codes[j] if with_codes else None, G)
                     for j, (G, _, with_codes) in enumerate(CALLS)]
        assert all(a.rc == 0 and a.res.code == 0 and a.res.n_values > ROWS // 2 for a in self.aggs)

    def arrays(self):
        """{name: the expected bytes}"""
        out = {}
        for j, a in enumerate(self.aggs):
            out.update({f"groups{j}": a.groups, f"res{j}": np.frombuffer(bytes(a.res), dtype=np.uint8)})
        return out


def test_expected_on_cpu():
    """A's and the decoy's expected arrays have the same sizes and differ in the records of every call: a call that read the
    decoy shows"""
    a, b = Expected(False), Expected(True)
    assert SENTINEL != tam.FILL
    for name, want in a.arrays().items():
        other = b.arrays()[name]
        assert want.size == other.size and not np.array_equal(want, other), name


class Tensors:
    """The inputs and the caller's output tensors of the three calls on one device"""

    def __init__(self, dev, x, start):
        import torch

        self.dev, self.x = dev, x
        self.d_rec = [ttd.to_device(dev, c.reshape(-1)).view(torch.int64).view(c.shape[0], ROWS, 2) for c in start.columns]
        self.d_codes = [torch.from_numpy(c).to(dev.device) for c in start.codes]
        self.d_sel = ttd.to_device(dev, np.frombuffer(bytes(tcm.select_result(ROWS)), dtype=np.uint8))
        self.out = {name: ttd.to_device(dev, np.full(w.size, tam.FILL, dtype=np.uint8)) for name, w in x.arrays().items()}
        self.pristine = {name: t.clone() for name, t in self.out.items()}

    def copy_in(self, other):
        for mine, theirs in zip(self.d_rec + self.d_codes, other.d_rec + other.d_codes):
            mine.copy_(theirs, non_blocking=True)

    def reset(self):
        for name, t in self.out.items():
            t.copy_(self.pristine[name], non_blocking=True)

    def call(self, j):
        G, _, with_codes = CALLS[j]
        self.dev.aggregate(self.d_rec[j], self.d_sel, self.d_codes[j] if with_codes else None, n_groups=G, d_groups=self.out[f"groups{j}"],
                           groups_capacity=G, d_result=self.out[f"res{j}"], sync=False)

    def check(self, want, where):
        for name, w in want.items():
            got = self.out[name].cpu().numpy()
            bad = np.nonzero(got != w)[0]
            assert bad.size == 0, (where, name, int(bad[0]) // 48, got[bad[:4]].tolist(), w[bad[:4]].tolist(), int(bad.size))


@pytest.mark.gpu
def test_aggregate_behind_late_inputs(dev):
    import time

    import torch

    a, b = Expected(False), Expected(True)
    t, source = Tensors(dev, a, b), Tensors(dev, a, a)

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
        t.copy_in(source)
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
            t.call(1)
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
