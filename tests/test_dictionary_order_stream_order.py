"""msj_dictionary_order_device and msj_rank_rows_device in stream order (the manner of tests/test_join_rows_stream_order.py; the
delay and its bounds are tests/test_stream_order.py's): on a side stream, behind a dictionary that arrives late, with
sync=False and every output a tensor of the caller's.

The decoy B -- A's sizes, other bytes -- lies in the dictionary tensors and has been through the calls: one whole order, an
order cut after one round, its continuation, and the rank records of a code column by it.  Every tensor and the workspace
hold B's consistent state.  Then, on a side stream: a delay, device-to-device copies of A's offsets and bytes over them, the
outputs back to their fill, and the calls.  A launch or a memset that dropped its stream argument runs ahead of the copies
and reads the decoy; what it writes is then overwritten with the fill or differs from A's expected arrays, which come from
the host twin alone.  With nullptr for `stream` at msj_launch_dictionary_order (tried once on a copy of the tree) the test fails at
the first order's `sorted0`, which still holds its fill: the kernels ran on the null stream ahead of the side stream's copies
and the reset.

The second set-up runs two contexts on two streams in turns, A on one and B on the other, with nothing waited for.
"""
import numpy as np
import pytest

from tests import test_dictionary_order_math as tdm
from tests import test_stream_order as tso
from tests import test_tape_documents as ttd

ROWS = 5000
SIZES = (3000, 1000)   # the grid path, the one-workgroup path


def make_values(seed, V):
    import random

    rng = random.Random(seed)
    return [b"host-" + tdm.word(rng, 7) for _ in range(V)]   # one length: A's and the decoy's offsets agree, a call's sizes too


class Expected:
    """The calls over one dictionary on the host"""

    def __init__(self, decoy, V):
        tw = tdm.load_twin()
        self.V, self.d = V, tdm.Dict(make_values(77 if decoy else 7, V))
        self.codes = np.random.default_rng(3).integers(-2, V + 1, ROWS).astype(np.int32)
        _, self.whole, self.s0, self.r0, _ = tdm.run_twin(tw, self.d, max_rounds=8)
        _, self.cut, s1, r1, _ = tdm.run_twin(tw, self.d, max_rounds=1)
        _, self.rest, self.s1, self.r1, _ = tdm.run_twin(tw, self.d, depth=8, max_rounds=8, flags=tdm.CONTINUE, state=(s1, r1))
        assert self.whole.code == 0 and self.cut.code == 1 and self.cut.n_tied > V // 2 and self.rest.code == 0
        assert np.array_equal(self.s0, self.s1) and np.array_equal(self.r0, self.r1)
        rc, self.rres, self.rsel, self.fields = tdm.run_rank_rows(tw, self.codes, self.r1, self.rest)
        assert rc == 0 and self.rres.code == 0 and self.rres.n_ranked > ROWS // 2

    def arrays(self):
        """{name: the expected bytes}, in the order of the calls"""
        raw = lambda s: np.frombuffer(bytes(s), dtype=np.uint8)
        return {"sorted0": self.s0.view(np.uint8), "rank0": self.r0.view(np.uint8), "res0": raw(self.whole), "res1": raw(self.cut),
                "sorted1": self.s1.view(np.uint8), "rank1": self.r1.view(np.uint8), "res2": raw(self.rest),
                "fields": np.frombuffer(self.fields.tobytes(), dtype=np.uint8), "rres": raw(self.rres), "rsel": raw(self.rsel)}


@pytest.mark.parametrize("V", SIZES)
def test_expected_on_cpu(V):
    """A's and the decoy's expected arrays have the same sizes and differ in every array a call writes but the counts: a call
    that read the decoy shows"""
    a, b = Expected(False, V), Expected(True, V)
    assert np.array_equal(a.d.offsets, b.d.offsets) and a.d.cap == b.d.cap and not np.array_equal(a.d.bytes, b.d.bytes)
    for name, want in a.arrays().items():
        other = b.arrays()[name]
        assert want.size == other.size and (name.startswith("r") and not name.startswith("rank") or not np.array_equal(want, other)), name


class Tensors:
    """The dictionary, the codes and the caller's output tensors of the calls on one device"""

    def __init__(self, dev, x, start):
        self.dev, self.x = dev, x
        self.d_offsets, self.d_bytes, self.d_codes = ttd.to_device(dev, start.d.offsets), ttd.to_device(dev, start.d.bytes), ttd.to_device(dev, x.codes)
        self.out = {name: ttd.to_device(dev, np.full(w.size, 0xA5, dtype=np.uint8)) for name, w in x.arrays().items()}
        self.pristine = {name: t.clone() for name, t in self.out.items()}

    def copy_in(self, other):
        self.d_offsets.copy_(other.d_offsets, non_blocking=True)
        self.d_bytes.copy_(other.d_bytes, non_blocking=True)

    def reset(self):
        for name, t in self.out.items():
            t.copy_(self.pristine[name], non_blocking=True)

    def call(self, j):
        import torch

        i32 = lambda name: self.out[name].view(torch.int32)
        dev, V = self.dev, self.x.V
        if j == 0:
            dev.dictionary_order(self.d_offsets, self.d_bytes, n_entries=V, capacity=V, max_rounds=8, d_sorted=i32("sorted0"), d_rank=i32("rank0"),
                                 d_result=self.out["res0"], sync=False)
        elif j == 1:
            dev.dictionary_order(self.d_offsets, self.d_bytes, n_entries=V, capacity=V, max_rounds=1, d_sorted=i32("sorted1"), d_rank=i32("rank1"),
                                 d_result=self.out["res1"], sync=False)
        elif j == 2:
            dev.dictionary_order(self.d_offsets, self.d_bytes, n_entries=V, capacity=V, depth=8, max_rounds=8, resume=True, d_sorted=i32("sorted1"),
                                 d_rank=i32("rank1"), d_result=self.out["res2"], sync=False)
        else:
            dev.rank_rows(self.d_codes, i32("rank1"), self.out["res2"], rank_capacity=V, d_fields=self.out["fields"].view(torch.int64).view(ROWS, 2),
                          d_result=self.out["rres"], d_select=self.out["rsel"], sync=False)

    def check(self, want, where):
        for name, w in want.items():
            got = self.out[name].cpu().numpy()
            bad = np.nonzero(got != w)[0]
            assert bad.size == 0, (where, name, int(bad[0]) // 4, got[bad[:4]].tolist(), w[bad[:4]].tolist(), int(bad.size))


N_CALLS = 4


@pytest.mark.gpu
@pytest.mark.parametrize("V", SIZES)
def test_order_behind_a_late_dictionary(dev, V):
    import time

    import torch

    a, b = Expected(False, V), Expected(True, V)
    t, source = Tensors(dev, a, b), Tensors(dev, a, a)

    def enqueue():
        t.reset()
        for j in range(N_CALLS):
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
    assert pending, "inconclusive: the dictionary was there when the enqueue returned -- a host wait in the call, or the delay too short: " + numbers
    assert delay_ms >= need_ms, numbers
    t.check(a.arrays(), "behind a late dictionary")


@pytest.mark.gpu
def test_two_contexts_two_streams():
    """Two contexts on two side streams, A on one and the decoy B on the other, the calls enqueued in turns with nothing waited
    for: device state that the process holds once would be shared by the two"""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    devs = [Stage1Device(0), Stage1Device(0)]
    try:
        windows = [Expected(False, SIZES[0]), Expected(True, SIZES[0])]
        sets = [Tensors(d, x, x) for d, x in zip(devs, windows)]
        for t in sets:   # every workspace has its size
            t.call(0)
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(d.device) for d in devs]
        for s, t in zip(streams, sets):
            with torch.cuda.stream(s):
                t.reset()
        for _ in range(3):
            for j in range(N_CALLS):
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
