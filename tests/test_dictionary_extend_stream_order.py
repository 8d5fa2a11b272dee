"""msj_dictionary_extend_device in stream order (the manner of tests/test_aggregate_stream_order.py; the delay and its bounds
are tests/test_stream_order.py's): a chain of three windows into one dictionary on a side stream, behind inputs that arrive
late, with sync=False, each call's P read on the device from the previous call's result, the capacities given and every
output a tensor of the caller's.

The decoy B -- A's sizes, other values, other null rows -- lies in the columns and has been through the chain: every tensor
and the workspace hold B's consistent state.  Then, on a side stream: a delay, device-to-device copies of A's columns over
them, the outputs back to their fill, and the chain.  A launch or a memset that dropped its stream argument runs ahead of
the copies and reads the decoy; what it writes is then overwritten with the fill or differs from A's expected arrays, which
come from the host twin (tests/dictionary_extend_math_host.cpp) alone.  max_probe, which is no function of the input, is
left out of the comparison.

The second set-up runs two contexts on two streams in turns, A on one and B on the other, with nothing waited for.
"""
import numpy as np
import pytest

from tests import test_dictionary_extend_math as txm
from tests import test_dictionary_math as tdc
from tests import test_stream_order as tso
from tests import test_tape_documents as ttd

SIZES = (700, 1, 300)          # rows of the three windows
WIDTH = 6                      # every value has this many bytes: A and the decoy have arrays of one size
CAPACITY, ROOM = 600, 600 * WIDTH
PROBE = slice(40, 48)          # max_probe in the 64-byte result


class Expected:
    """The chain over one set of columns on the host"""

    def __init__(self, decoy):
        rng = np.random.default_rng(77 if decoy else 76)
        vocabulary = 420 if decoy else 300
        self.columns = []
        for size in SIZES:
            picks = rng.integers(0, vocabulary, size)
            values = [None if rng.integers(0, 9) == 0 else b"%0*d" % (WIDTH, (7 if decoy else 3) * int(p)) for p in picks]
            offsets = np.arange(size + 1, dtype=np.uint64) * WIDTH   # (a null row keeps its bytes' room: one size for A and B)
            data = b"".join(v if v is not None else b"-" * WIDTH for v in values)
            self.columns.append(tdc.Column(offsets, [v is not None for v in values], data))
        xtwin = txm.load_twin()
        arrays = txm.Arrays([], b"", CAPACITY, ROOM)
        self.out, P = {}, 0
        for j, col in enumerate(self.columns):
            res, codes = txm.twin_extend(xtwin, col, arrays, 0, p_word=P)
            assert res.code == 0 and res.n_prior == P
            P = int(res.n_distinct)
            self.out.update({f"codes{j}": codes.view(np.uint8).copy(), f"res{j}": np.frombuffer(bytes(res), dtype=np.uint8).copy()})
        self.out.update({"offsets": arrays.offsets.view(np.uint8), "first": arrays.first.view(np.uint8), "bytes": arrays.bytes})
        self.n_distinct = P

    def arrays(self):
        """{name: the expected bytes}"""
        return self.out


def test_expected_on_cpu():
    """A's and the decoy's expected arrays have the same sizes and differ in every one: a call that read the decoy shows"""
    a, b = Expected(False), Expected(True)
    assert 200 < a.n_distinct < b.n_distinct < CAPACITY
    for name, want in a.arrays().items():
        other = b.arrays()[name]
        assert want.size == other.size and not np.array_equal(want, other), name


class Tensors:
    """The columns and the caller's output tensors of the chain on one device"""

    def __init__(self, dev, x, start):
        import torch

        self.dev, self.x = dev, x
        self.cols = [(ttd.to_device(dev, c.offsets.view(np.int64)), ttd.to_device(dev, c.data), ttd.to_device(dev, c.valid)) for c in start.columns]
        self.out = {name: ttd.to_device(dev, np.full(w.size, tdc.FILL, dtype=np.uint8)) for name, w in x.arrays().items()}
        self.pristine = {name: t.clone() for name, t in self.out.items()}
        self.d_off, self.d_first = self.out["offsets"].view(torch.int64), self.out["first"].view(torch.int32)

    def copy_in(self, other):
        for mine, theirs in zip(self.cols, other.cols):
            for m, t in zip(mine, theirs):
                m.copy_(t, non_blocking=True)

    def reset(self):
        for name, t in self.out.items():
            t.copy_(self.pristine[name], non_blocking=True)

    def call(self, j):
        """Window j against the dictionary as the calls in front of it left it: P is the previous result's n_distinct"""
        import torch

        offsets, data, valid = self.cols[j]
        d_n_prior = self.out[f"res{j - 1}"][24:32].view(torch.int64) if j else None
        self.dev.dictionary_extend(offsets, data, valid, self.d_off, self.d_first, self.out["bytes"], d_n_prior=d_n_prior, rows=SIZES[j],
                                   bytes_len=SIZES[j] * WIDTH, d_codes=self.out[f"codes{j}"].view(torch.int32), dict_capacity=CAPACITY,
                                   dict_bytes_capacity=ROOM, d_result=self.out[f"res{j}"], sync=False)

    def chain(self):
        for j in range(len(SIZES)):
            self.call(j)

    def check(self, want, where):
        for name, w in want.items():
            got = self.out[name].cpu().numpy()
            if name.startswith("res"):
                got, w = got.copy(), w.copy()
                got[PROBE] = w[PROBE] = 0
            bad = np.nonzero(got != w)[0]
            assert bad.size == 0, (where, name, int(bad[0]), got[bad[:4]].tolist(), w[bad[:4]].tolist(), int(bad.size))


@pytest.mark.gpu
def test_chain_behind_late_inputs(dev):
    import time

    import torch

    a, b = Expected(False), Expected(True)
    t, source = Tensors(dev, a, b), Tensors(dev, a, a)

    def enqueue():
        t.reset()
        t.chain()

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    enqueue()   # the decoy through the chain: the workspace has its size and holds its state
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
    """Two contexts on two side streams, A on one and the decoy B on the other, the chains enqueued in turns with nothing
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
            t.chain()
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(d.device) for d in devs]
        for s, t in zip(streams, sets):
            with torch.cuda.stream(s):
                t.reset()
        for _ in range(3):
            for j in range(len(SIZES)):
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
