"""msj_sort_rows_device in stream order (the manner of tests/test_aggregate_stream_order.py; the delay and its bounds are
tests/test_stream_order.py's): on a side stream, behind inputs that arrive late, with sync=False, the capacities given and
every output a tensor of the caller's.

The decoy B -- A's sizes, other values and another row list -- lies in the records and in the list, and has been through the
three calls (the full sort, the selection, a sort of d_rows_in): every tensor and the workspace hold B's consistent state.
Then, on a side stream: a delay, device-to-device copies of A's records and row list over them, the outputs back to their
fill, and the calls.  A launch or a memset that dropped its stream argument runs ahead of the copies and reads the decoy;
what it writes is then overwritten with the fill or differs from A's expected arrays, which come from the host twin
(tests/sort_rows_math_host.cpp) alone.  With nullptr for `stream` at msj_launch_sort_rows (tried once on a copy of the tree,
with the first set-up) the test fails at the array "order0": the kernels ran on the null stream ahead of the side stream's
copies, and the side stream's reset of the outputs then left the fill where A's order belongs.

The second set-up runs two contexts on two streams in turns, A on one and B on the other, with nothing waited for.
"""
import numpy as np
import pytest

from tests import test_sort_rows_math as tsm
from tests import test_stream_order as tso
from tests import test_string_column_math as tcm
from tests import test_tape_documents as ttd

ROWS = 5000
LISTED = 3000
CALLS = ((1, 0, 0, False), (2, tsm.DESC, 300, False), (0, tsm.VALUES_ONLY, 0, True))     # mode, flags, limit, with d_rows_in
FILL32 = tsm.FILL32


def make_column(seed):
    from tests import test_sort_rows as tsr

    rng = np.random.default_rng(seed)
    k = np.arange(ROWS)
    col = tsr.pick(k % 3 == 0, tsr.doubles(rng.integers(-500, 500, ROWS) * 0.5), tsr.ints(rng.integers(-250, 250, ROWS)))
    return tsr.without_values(col, 7, 3), rng.integers(0, ROWS + 30, LISTED).astype(np.uint32)


class Expected:
    """The three calls over one column and one row list on the host"""

    def __init__(self, decoy):
        stw = tsm.load_twin()
        self.col, self.rows_in = make_column(77 if decoy else 7)
        self.sorted = [tsm.twin_sort(stw, self.col, ROWS, self.rows_in if listed else None, flags=flags, limit=limit)
                       for _, flags, limit, listed in CALLS]
        assert all(s.rc == 0 and s.res.code == 0 and s.res.n_written >= 300 for s in self.sorted)

    def arrays(self):
        """{name: the expected bytes}"""
        out = {}
        for j, s in enumerate(self.sorted):
            out.update({f"order{j}": s.order.view(np.uint8), f"res{j}": np.frombuffer(bytes(s.res), dtype=np.uint8),
                        f"select{j}": np.frombuffer(bytes(s.order_sel), dtype=np.uint8)})
        return out


def test_expected_on_cpu():
    """A's and the decoy's expected arrays have the same sizes and differ in the order of every call: a call that read the
    decoy shows"""
    a, b = Expected(False), Expected(True)
    for name, want in a.arrays().items():
        other = b.arrays()[name]
        assert want.size == other.size and (not name.startswith("order") or not np.array_equal(want, other)), name


class Tensors:
    """The inputs and the caller's output tensors of the three calls on one device"""

    def __init__(self, dev, x, start):
        import torch

        self.dev, self.x = dev, x
        self.d_rec = ttd.to_device(dev, start.col).view(torch.int64).view(ROWS, 2)
        self.d_rows_in = ttd.to_device(dev, start.rows_in)
        self.d_sel = ttd.to_device(dev, np.frombuffer(bytes(tcm.select_result(ROWS)), dtype=np.uint8))
        self.d_in_sel = ttd.to_device(dev, np.frombuffer(bytes(tcm.select_result(LISTED)), dtype=np.uint8))
        self.out = {name: ttd.to_device(dev, np.full(w.size, tsm.FILL, dtype=np.uint8)) for name, w in x.arrays().items()}
        self.pristine = {name: t.clone() for name, t in self.out.items()}

    def copy_in(self, other):
        self.d_rec.copy_(other.d_rec, non_blocking=True)
        self.d_rows_in.copy_(other.d_rows_in, non_blocking=True)

    def reset(self):
        for name, t in self.out.items():
            t.copy_(self.pristine[name], non_blocking=True)

    def call(self, j):
        import torch

        mode, flags, limit, listed = CALLS[j]
        self.dev.set_sort_mode(mode)
        self.dev.sort_rows(self.d_rec, self.d_sel, self.d_rows_in if listed else None, self.d_in_sel if listed else None,
                           descending=bool(flags & tsm.DESC), values_only=bool(flags & tsm.VALUES_ONLY), limit=limit,
                           capacity=LISTED if listed else ROWS, d_order=self.out[f"order{j}"].view(torch.int32), d_result=self.out[f"res{j}"],
                           d_order_select=self.out[f"select{j}"], sync=False)

    def check(self, want, where):
        for name, w in want.items():
            got = self.out[name].cpu().numpy()
            bad = np.nonzero(got != w)[0]
            assert bad.size == 0, (where, name, int(bad[0]) // 4, got[bad[:4]].tolist(), w[bad[:4]].tolist(), int(bad.size))


@pytest.mark.gpu
def test_sort_rows_behind_late_inputs(dev):
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
